"""The workgroup -> tile map of the GEMM / conv family, restated in numpy, and the small cases that take it past one
super-row (tests/test_tile_map_host.py checks the restatement and the cases on the CPU, tests/test_tile_map_gpu.py
runs the cases; tests/env_switches.py re-runs them under MIXDQ_IGEMM_GM).

What the three sites say in their comments (csrc/igemm_kernel.h "XCD- and L2-aware tile map", csrc/igemm_pp.h "this
workgroup's share of the tile sequence", csrc/iconv.hip "XCD-aware tile map"), and nothing of their expressions:

  * the tiles of a launch form one SEQUENCE: super-rows of `gm` m-tiles, one after the other; inside a super-row the
    m-tile runs fastest, then the n-tile; the last super-row holds what is left of tiles_m (1 .. gm m-tiles);
  * the hardware deals workgroups round-robin over 8 XCDs (workgroup b lands on XCD b % 8, as that XCD's (b // 8)-th);
    every XCD owns one CONTIGUOUS RUN of the sequence, the runs in XCD order, their lengths as equal as they can be:
    the first (tiles % 8) XCDs hold one tile more;
  * one workgroup per tile: the (b // 8)-th workgroup of an XCD computes the (b // 8)-th tile of that XCD's run;
  * persistent form (G workgroups, G % 8 == 0): the G / 8 workgroups of an XCD take the tiles of its run round-robin:
    workgroup b takes elements b // 8, b // 8 + G / 8, b // 8 + 2 G / 8, ... of the run.

Imports without a GPU and without the built library.
"""
import os
import re

import numpy as np

from tests import tile_edges as te

XCDS = 8
GM_DEFAULT = 8
PATHS = ("second_super_row", "partial_super_row", "uneven_runs")


def gm_rule(value):
    """csrc/igemm_kernel.h tile_map_gm: MIXDQ_IGEMM_GM inside 1..64, else 8."""
    return value if 1 <= value <= 64 else GM_DEFAULT


# ------------------------------------------------------------------------------------------------ the restatement
def sequence(tiles_m, tiles_n, gm):
    """[tiles, 2] int: the (m-tile, n-tile) of every element of the tile sequence, built by walking it."""
    out = []
    for first in range(0, tiles_m, gm):
        rows = range(first, min(first + gm, tiles_m))
        for n in range(tiles_n):
            for m in rows:
                out.append((m, n))
    return np.asarray(out, np.int64).reshape(-1, 2)


def runs(tiles):
    """[(start, end)] of the 8 XCDs' runs of a sequence of `tiles` elements."""
    lens = [tiles // XCDS + (1 if x < tiles % XCDS else 0) for x in range(XCDS)]
    starts = np.concatenate([[0], np.cumsum(lens)])
    return [(int(starts[x]), int(starts[x + 1])) for x in range(XCDS)]


def seq_of(bid, tiles):
    """Sequence index of workgroup `bid` of a one-workgroup-per-tile launch of `tiles` workgroups."""
    start, end = runs(tiles)[bid % XCDS]
    s = start + bid // XCDS
    assert s < end, "a launch of `tiles` workgroups gives XCD x exactly its run's length"
    return s


def tile_of(bid, tiles_m, tiles_n, gm=GM_DEFAULT):
    """(m-tile, n-tile) workgroup `bid` computes."""
    m, n = sequence(tiles_m, tiles_n, gm)[seq_of(bid, tiles_m * tiles_n)]
    return int(m), int(n)


def persistent_seq(bid, k, grid, tiles):
    """Sequence index of the k-th tile of workgroup `bid` of a persistent launch of `grid` workgroups, or None when
    that workgroup has fewer tiles."""
    assert grid % XCDS == 0 and 0 <= bid < grid
    start, end = runs(tiles)[bid % XCDS]
    s = start + bid // XCDS + k * (grid // XCDS)
    return s if s < end else None


def persistent_grid(tiles, cus=256, cap=None):
    """csrc/igemm_pp.h launch_pp: one workgroup per CU in whole XCD rounds, capped by MIXDQ_IGEMM_PERSIST_WGS (whole
    rounds, at least one), never more rounds than the tiles need."""
    grid = cus // XCDS * XCDS
    if cap is not None and XCDS <= cap // XCDS * XCDS < grid:
        grid = cap // XCDS * XCDS
    return min(grid, -(-tiles // XCDS) * XCDS)


def paths(tiles_m, tiles_n, gm=GM_DEFAULT):
    """Which of the map's three branches a launch reaches: a second super-row (a workgroup whose super-row does not
    start at m-tile 0), a partial last super-row (fewer than gm m-tiles), XCD runs of unequal length longer than one
    tile (tiles % 8 != 0 with tiles >= 8: the two arms of the run formula differ and bid // 8 > 0 occurs)."""
    tiles = tiles_m * tiles_n
    return {PATHS[0]: tiles_m > gm, PATHS[1]: tiles_m % gm != 0, PATHS[2]: tiles % XCDS != 0 and tiles // XCDS >= 1}


# ------------------------------------------------------------------------------------------------ the sites
# file -> what of the map it holds.  tests/test_tile_map_host.py holds this equal to the files of csrc/ that contain the
# run formula ("... % kNumXCD"): a further copy needs a row -- and cases.
SITES = {
    "igemm_kernel.h": dict(form="one workgroup per tile", gm="p.gm (MIXDQ_IGEMM_GM)",
                           families=("linear_fast", "linear_generic", "w4", "w2", "geglu", "conv", "f16", "grouped",
                                     "f16in", "ln_global", "ln_local", "pp70")),
    "igemm_pp.h": dict(form="persistent: runs taken round-robin by G / 8 workgroups", gm="p.gm (MIXDQ_IGEMM_GM)",
                       families=("pp71",)),
    "iconv.hip": dict(form="one workgroup per tile", gm="constexpr 8",
                      families=("halo90", "halo91", "halo92", "halo93", "halo90_ups", "halo91_w4", "halo92_w4")),
    # the run formula alone, over (batch x head x query block) with no super-rows: not this map.  Its own switch has
    # its own test (tests/env_switches.py MIXDQ_ATTN_XCD).
    "attention.hip": dict(form="run formula only (no super-rows)", gm=None, families=()),
}
RUN_FORMULA = re.compile(r"%\s*kNumXCD\b")          # (whatever the copy calls its quotient and remainder)


def census(csrc=te.CSRC):
    """Files of csrc/ that hold the run formula."""
    found = set()
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            text = open(os.path.join(csrc, name)).read()
            if RUN_FORMULA.search(text):
                found.add(name)
    return found


# ------------------------------------------------------------------------------------------------ the cases
# One configuration per family (the per-configuration sweep is tests/test_tile_edges_gpu.py under MIXDQ_IGEMM_GM = 1, 2:
# tests/env_switches.py).  Smallest shapes that reach the paths: tiles_m in {9, 11} (a last super-row of 1 and of 3),
# tiles_n in {1, 3}: 9, 11, 27, 33 workgroups (8 q8 + {1, 3}); M = tiles_m BM - 5, N = tiles_n BN - 4 (GEGLU: - 32,
# whole value|gate groups), K two K-tiles unless the form says otherwise.
TILES_M, TILES_N = (9, 11), (1, 3)
HALO = te._xmacro(os.path.join(te.CSRC, "iconv.h"), "MIXDQ_HALO_TILES")     # id -> (TH, TW, BN, CK, WNG)

# family -> (table, configuration, what the K of the case is)
GEMM_FAMILIES = {
    "linear_fast": (te.IGEMM, 1, "two K-tiles: K % BK == 0, the LDS-DMA staging path"),
    "linear_generic": (te.IGEMM, 35, "two K-tiles less 16: K % BK != 0, the generic staging path"),
    "w4": (te.IGEMM, 41, "two K-tiles of packed 4-bit weights"),
    "w2": (te.IGEMM, 37, "two K-tiles of packed 2-bit weights (a k-split tile)"),
    "geglu": (te.IGEMM, 3, "two K-tiles; N in whole 32-column value|gate groups"),
    "conv": (te.IGEMM, 4, "3x3 pad 1 on 16 channels: K = 144, taps straddle the K-tiles"),
    "f16": (te.F16, 4, "two K-tiles of FP16 (BK counts bytes)"),
    "grouped": (te.GROUPED, 4, "two members, N = BN - 4 and 3 BN - 4: the narrow one leaves workgroups idle"),
    "f16in": (te.AQ, 13, "two K-tiles of FP16 activations quantized in the prologue"),
    "pp70": (te.IGEMM, 70, "two K-tiles, the four-phase 256 x 256 tile"),
    "pp71": (te.IGEMM, 71, "two K-tiles, the persistent form (N % 8 == 0, else the launch runs 70's kernel)"),
}
# GEMM + LayerNorm (csrc/igemm_ln.hip, tile 56: 64 x 80): a column tile is one unit of the LayerNorm, so N fixes
# tiles_n: N = 640, eight column tiles: 72 and 88 workgroups, under the one-round residency limit, tiles % 8 == 0; and
# N = 320, four column tiles: 36 and 44 workgroups (8 q8 + 4: uneven runs).  Global records (K > 2048): the super-row
# map.  Local records (K <= 2048): a row-major order behind the same run formula.
LN_CFG = 56
LN_WIDTHS = (320, 640)
LN_FORMS = {"ln_global": dict(K=2176), "ln_local": dict(K=256)}


def _gemm_case(family, tm, tn):
    table, cfg, _ = GEMM_FAMILIES[family]
    bm, bn, bk, st = te.tile(cfg, table)
    c = dict(family=family, cfg=cfg, BM=bm, BN=bn, tiles_m=tm, tiles_n=tn, M=tm * bm - 5, N=tn * bn - 4, K=2 * bk)
    if family == "linear_generic":
        c["K"] = 2 * bk - 16
    elif family == "geglu":
        c["N"] = tn * bn - 32
    elif family == "f16":
        c["K"] = 2 * bk // 2                     # elements
    elif family == "pp71":
        c["N"] = tn * bn - 8
    elif family == "grouped":
        c["Ns"] = [bn - 4, tn * bn - 4]          # member 0: one column tile; member 1: tn of them (the grid's width)
    elif family == "conv":
        # M = H W output pixels of one image (3x3, stride 1, pad 1): 571 = 571 x 1, 699 = 233 x 3
        H, W = {571: (571, 1), 699: (233, 3)}[c["M"]]
        c.update(H=H, W=W, C=16, K=9 * 16)
    return c


def _ln_case(family, tm, N):
    return dict(family=family, cfg=LN_CFG, BM=64, BN=80, tiles_m=tm, tiles_n=N // 80, M=tm * 64 - 5, N=N,
                K=LN_FORMS[family]["K"])


def _halo_case(family, images):
    tile = int(family[4:6])
    th, tw, bn, ck, wng = HALO[tile]
    # 3 x 3 whole tiles per image: 9 and 18 pixel tiles (super-rows 8 + 1 and 8 + 8 + 2); two channel tiles
    return dict(family=family, cfg=tile, TH=th, TW=tw, BN=bn, n=images, H=3 * th, W=3 * tw, C=128, K=2 * bn - 4,
                tiles_m=images * 9, tiles_n=2, ups=family.endswith("_ups"), w4=family.endswith("_w4"))


def cases():
    out = []
    for family in GEMM_FAMILIES:
        out += [_gemm_case(family, tm, tn) for tm in TILES_M for tn in TILES_N]
    for family in LN_FORMS:
        out += [_ln_case(family, tm, N) for tm in TILES_M for N in LN_WIDTHS]
    for family in SITES["iconv.hip"]["families"]:
        out += [_halo_case(family, n) for n in (1, 2)]
    return out


CASES = cases()
FAMILIES = sorted({c["family"] for c in CASES})
# ln_local replaces the super-rows by a row-major order (csrc/igemm_kernel.h, LNQ): it has the run formula only
REQUIRED = {f: (PATHS[2:] if f == "ln_local" else PATHS) for f in FAMILIES}


def case_id(c):
    if c["family"].startswith("halo"):
        return f"{c['family']}_n{c['n']}_{c['H']}x{c['W']}_c{c['C']}_k{c['K']}"
    return f"{c['family']}_cfg{c['cfg']}_m{c['M']}_n{c['N']}_k{c['K']}"


def case_tiles(c):
    """(tiles_m, tiles_n) of a case, from its extents and its tile (not from the fields it was built with)."""
    if c["family"].startswith("halo"):
        return c["n"] * (c["H"] // c["TH"]) * (c["W"] // c["TW"]), -(-c["K"] // c["BN"])
    n = max(c["Ns"]) if "Ns" in c else c["N"]
    return -(-c["M"] // c["BM"]), -(-n // c["BN"])


def reached(family, gm=GM_DEFAULT):
    """Paths the cases of a family reach, together."""
    got = {p: False for p in PATHS}
    for c in CASES:
        if c["family"] == family:
            g = GM_DEFAULT if SITES["iconv.hip"]["families"].count(family) else gm       # the halo map's is constexpr
            for p, v in paths(*case_tiles(c), g).items():
                got[p] = got[p] or v
    return got


# ------------------------------------------------------------------------------------------------ index-coded operands
# Operands whose exact product names the tile it belongs to: out[m, n] = code(m-tile, n-tile) with
# code = 1 + tm + 13 (1 + tn) (tm <= 12: distinct for every tile of every case), scale 1, bias0 0, no bias.  A tile
# computed in another tile's place, twice, or not at all changes an integer -- random data could hide a swap of two tiles
# only by accident, but two wrong tiles cannot cancel here.  a[m] = (1 + tm, 13, 0 ...), w[n] = (1, 1 + tn, filler ...).
def tile_code(tm, tn):
    return 1 + tm + 13 * (1 + tn)


def _exact_product(a, w):
    """a w^T of int8 operands as int64, through float64 (exact: |sum| <= K 2^14 < 2^53; an int64 matmul has no BLAS)."""
    assert a.shape[1] <= 1 << 30
    return np.rint(a.astype(np.float64) @ w.astype(np.float64).T).astype(np.int64)


def coded_gemm(M, N, K, bm, bn, seed=0):
    """a int8 [M, K], w int8 [N, K] in [-2, 1] (packs to W4 and W2), acc int64 [M, N] == tile_code of its tile."""
    from tests import detdata as dd
    assert K >= 2 and (M - 1) // bm <= 12 and 1 + (N - 1) // bn <= 9
    a = np.zeros((M, K), np.int8)
    a[:, 0] = 1 + np.arange(M) // bm
    a[:, 1] = 13
    w = np.array([-2, -1, 1], np.int8)[(dd.u64(977 + seed, N * K) % np.uint64(3)).astype(np.int64)].reshape(N, K)
    w[:, 0] = 1
    w[:, 1] = 1 + np.arange(N) // bn             # <= 9 ... as W2 (range [-2, 1]) only 1: see coded_gemm_w2
    acc = _exact_product(a, w)
    want = tile_code(np.arange(M)[:, None] // bm, np.arange(N)[None, :] // bn)
    assert np.array_equal(acc, want)
    return a, w, acc


def coded_gemm_narrow(M, N, K, bm, bn, seed=0):
    """As coded_gemm with weights in [-2, 1] throughout (packed W2): the n-tile's term is spread over 1 + tn columns of
    weight 1 against a[m] = 13 there.  Needs K >= 2 + tiles_n."""
    from tests import detdata as dd
    tn_max = (N - 1) // bn
    assert K >= 2 + tn_max
    a = np.zeros((M, K), np.int8)
    a[:, 0] = 1 + np.arange(M) // bm
    a[:, 1:2 + tn_max] = 13
    w = np.array([-2, -1, 1], np.int8)[(dd.u64(979 + seed, N * K) % np.uint64(3)).astype(np.int64)].reshape(N, K)
    w[:, 0] = 1
    for j in range(tn_max + 1):
        w[:, 1 + j] = (np.arange(N) // bn >= j).astype(np.int8)
    acc = _exact_product(a, w)
    assert np.array_equal(acc, tile_code(np.arange(M)[:, None] // bm, np.arange(N)[None, :] // bn))
    return a, w, acc


def coded_conv(n, H, W, C, K, pixel_tile, bn, lo=-128):
    """x int8 [n, H, W, C], w int8 [K, 3, 3, C] with the centre tap alone non-zero in channels 0 and 1: the 3x3 / pad 1
    accumulator of output pixel (i, y, x), channel k is tile_code(pixel_tile[i, y, x], k // bn).  The other channels
    of x hold filler that meets zero weights."""
    from tests import detdata as dd
    assert C >= 2 and pixel_tile.shape == (n, H, W) and pixel_tile.max() <= 100 and (K - 1) // bn <= 5
    x = dd.int8(981, (n, H, W, C), max(lo, -8), 8)
    x[..., 0] = 1 + pixel_tile
    x[..., 1] = 13
    w = np.zeros((K, 3, 3, C), np.int8)
    w[:, 1, 1, 0] = 1
    w[:, 1, 1, 1] = 1 + np.arange(K) // bn
    acc = tile_code(pixel_tile[..., None], (np.arange(K) // bn)[None, None, None, :]).astype(np.int64)
    return x, w, acc
