"""Conv cases away from 3x3 / 1x1, and an independent numpy reference of the INT8 conv (tests/test_conv_geometry_gpu.py
runs them on the GPU; tests/test_conv_geometry_host.py checks the coverage and the reference on the CPU).

The conv entry points take any (R, S, stride, pad) -- the INT8 ones with pad < R and pad < S -- and the code that
depends on the geometry (the implicit-GEMM gather's tap stepping, the border-class index
((rlo * R + rhi) * S + slo) * S + shi in its four copies, the zero-point propagation) is written for R != S and pad > 1.
A transposed R / S is invisible at R == S and a clamp error at pad == 1: GEOMETRIES leaves both.

Per geometry three images: `tiny` (smaller than the window wherever the padding allows it: a pixel meets the first and
the last border at once), `full` (within 11 x 9, (H + 2 pad - R) % stride == 0: an interior and all four borders) and
`ragged` (one row and one column less, batch 3: a stride remainder != 0 under every stride > 1).
Channels: 16 (several taps per K-tile), 48 (taps straddle a 128-byte K-tile off a multiple of 16), 320; 4 and 20 (the
one-output-per-thread generic kernel); packed W4: 32, 64, 320.  Output channels: BN + 4 and 2 BN - 4 of the tile in use.
Tiles: one configuration per distinct value of every template parameter the activation gather depends on (a greedy
cover of the X-macro tables, read as tests/tile_edges.py reads them), and the automatic choice.  The values are
covered, not multiplied: case i of a geometry cycles images and tiles with co-prime steps.

Imports without a GPU and without the built library.
"""
import functools

import numpy as np

from tests import detdata as dd
from tests import exact_inputs as ei
from tests import tile_edges as te

# (R, S, stride, pad); the last is the control
GEOMETRIES = [(1, 3, 1, 0), (3, 1, 1, 0), (3, 1, 2, 0), (2, 2, 1, 1), (2, 2, 2, 0), (4, 4, 2, 1), (3, 3, 1, 2),
              (3, 3, 3, 1), (5, 5, 1, 2), (5, 5, 2, 2), (3, 5, 1, 2), (5, 3, 2, 1), (7, 7, 2, 3), (3, 3, 1, 1)]
# pad >= R or pad >= S: MIXDQ_ERR_PADDING on the INT8 entries (a window with no tap inside the image has no border
# class); mixdq_conv2d_f16 runs them (zero padding needs no class)
REFUSED = [(1, 3, 1, 1), (3, 3, 1, 3), (2, 2, 1, 2)]
C_INT8 = (16, 48, 320, 4, 20)
C_GENERIC = (4, 20)
C_W4 = (32, 64, 320)
C_F16 = (8, 24, 64, 4)              # 4: C % 8 != 0, the FP16 generic kernel
ZP = -11.0


def out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def _whole(extent, size, stride, pad):
    """The largest extent' <= extent whose padded length is a whole number of strides past the window."""
    return extent - (extent + 2 * pad - size) % stride


def images(R, S, stride, pad):
    """[(name, n, H, W)] of one geometry: `full` is the largest image within 11 x 9 with no stride remainder in either
    direction (the last window ends in the padding: a bottom and a right border), `ragged` one row and one column
    less (remainder stride - 1: the last padding rows are never read)."""
    tiny = (max(1, R - 2 * pad), max(1, S - 2 * pad) + (1 if pad else 0))
    H, W = _whole(11, R, stride, pad), _whole(9, S, stride, pad)
    return [("tiny", 1, *tiny), ("ragged", 3, H - 1, W - 1), ("full", 1, H, W)]


def stride_remainder(H, R, stride, pad):
    return (H + 2 * pad - R) % stride


# ------------------------------------------------------------------------------------------------ tiles
def _cover(rows):
    """Greedy cover: ids of `rows` ({id: tuple of gather parameters}) such that every value of every parameter
    occurs; deterministic (most new values first, lowest id on ties)."""
    need = {(i, v) for vals in rows.values() for i, v in enumerate(vals)}
    chosen = []
    while need:
        best = max(sorted(rows), key=lambda c: len(need & set(enumerate(rows[c]))))
        chosen.append(best)
        need -= set(enumerate(rows[best]))
    return sorted(chosen)


def _igemm_gather_params():
    """id -> (BM, BK, STAGES, waves, KSPLIT, MT, PHASED): what decides which 16-byte chunk of which tap a lane
    stages for which K-tile (rows per tile, K-tile bytes, pipeline depth, chunks per wave, k-split groups, MFMA shape
    / phase variant)."""
    import os
    import re
    text = open(os.path.join(te.CSRC, "igemm.hip")).read()
    m = re.search(r"#define\s+MIXDQ_IGEMM_CONFIGS\(X\)(.*?)\n(?!\s*X\()", text + "\n", flags=re.S)
    out = {}
    for args in re.findall(r"X\(([^)]*)\)", m.group(1)):
        v = [a.strip() for a in args.split(",")]
        cid, bm, bn, bk, st, wm, wn, ks, mt = (int(a) for a in v[:9])
        out[cid] = (bm, bk, st, wm * wn * ks, ks, mt, v[9] == "true")
    assert sorted(out) == sorted(te.IGEMM)
    return out


IGEMM_GATHER = _igemm_gather_params()
F16_GATHER = {c: (v[0], v[2], v[3], v[4] * v[5] * v[6], v[6], v[7]) for c, v in te.F16.items()}
TILES = [0] + _cover(IGEMM_GATHER)          # 0: the automatic choice
TILES_F16 = [0] + _cover(F16_GATHER)


def tile_bn(cfg, table=None):
    return te.tile(cfg, table)[1] if cfg else 64


# ------------------------------------------------------------------------------------------------ cases
def _case(form, i, g, C, cfg, img, table=None):
    R, S, stride, pad = g
    name, n, H, W = img
    bn = tile_bn(cfg, table)
    P, Q = out_hw(H, W, R, S, stride, pad)
    return dict(form=form, R=R, S=S, stride=stride, pad=pad, image=name, n=n, H=H, W=W, P=P, Q=Q, C=C, cfg=cfg,
                K=bn + 4 if i % 2 == 0 else 2 * bn - 4, bias=i % 2 == 0,
                residual=("", "full", "image")[i % 3] if i % 4 == 1 else "")


def _cases(form, geoms, channels, tiles, table=None):
    out, i = [], 0
    for gi, g in enumerate(geoms):
        imgs = images(*g)
        for ci, C in enumerate(channels):
            img = imgs[(ci + gi) % 3]           # every image of a geometry, each channel class on all of them in turn
            cfg = 0 if C in C_GENERIC and form == "w8" else tiles[i % len(tiles)]
            out.append(_case(form, i, g, C, cfg, img, table))
            i += 1
    return out


INT8_CASES = _cases("w8", GEOMETRIES, C_INT8, TILES)
W4_CASES = _cases("w4", GEOMETRIES, C_W4, TILES)
F16_CASES = _cases("f16", GEOMETRIES + REFUSED, C_F16, TILES_F16, te.F16)
RS = sorted({(g[0], g[1]) for g in GEOMETRIES})


def case_id(c):
    return (f"{c['form']}_{c['R']}x{c['S']}_s{c['stride']}_p{c['pad']}_{c['image']}_n{c['n']}_{c['H']}x{c['W']}"
            f"_c{c['C']}_k{c['K']}_t{c['cfg']}_{'bias' if c['bias'] else 'nobias'}"
            + (f"_{c['residual']}" if c["residual"] else ""))


def _seed(c):
    s = 29
    for v in (c["R"], c["S"], c["stride"], c["pad"], c["n"], c["H"], c["W"], c["C"], c["K"]):
        s = (s * 1000003 + int(v)) % (1 << 31)
    return s


def inputs(c):
    """x [n, H, W, C] int8 over the whole range, w [K, R, S, C] (W4: [-8, 7]), scale, bias, residual (NHWC order)."""
    s = _seed(c)
    x = dd.int8(s, (c["n"], c["H"], c["W"], c["C"]))
    lo, hi = (-8, 8) if c["form"] == "w4" else (-128, 128)
    w = dd.int8(s + 1, (c["K"], c["R"], c["S"], c["C"]), lo, hi)
    for a, (amin, amax) in ((x, (-128, 127)), (w, (lo, hi - 1))):       # both ends of the range, also in a tiny tensor
        a.reshape(-1)[0], a.reshape(-1)[-1] = amin, amax
    scale = dd.f32(s + 2, (c["K"],), 1e-4, 6e-4)
    bias = dd.f16(s + 3, (c["K"],), -1, 1) if c["bias"] else None
    res = None
    if c["residual"] == "full":
        res = dd.normal_f16(s + 4, (c["n"], c["P"], c["Q"], c["K"]), 2.0)
    elif c["residual"] == "image":
        res = dd.normal_f16(s + 4, (c["n"], c["K"]), 2.0)
    return dict(x=x, w=w, scale=scale, bias=bias, residual=res)


# ------------------------------------------------------------------------------------------------ reference
def window(p, size, extent, stride, pad):
    """Taps [lo, hi] (inclusive; hi < lo: none) of the window of output index p that fall inside [0, extent)."""
    b = p * stride - pad
    return max(0, -b), min(size - 1, extent - 1 - b)


def border_classes(R, S, stride, pad, H, W):
    """{(rlo, rhi, slo, shi)} of every output pixel, by window intersection."""
    P, Q = out_hw(H, W, R, S, stride, pad)
    return {window(p, R, H, stride, pad) + window(q, S, W, stride, pad) for p in range(P) for q in range(Q)}


def class_index(R, S, rlo, rhi, slo, shi):
    """Row of mixdq_conv_border_table (include/mixdq_hip.h)."""
    return ((rlo * R + rhi) * S + slo) * S + shi


def rect_sum(wsum, rlo, rhi, slo, shi):
    """float32 sum of wsum[:, r, s] over the rectangle ([K]; zeros for an empty one).  Exact in any order: the tap sums
    are integers and so is every partial sum, all below 2^24 (asserted)."""
    part = wsum[:, rlo:rhi + 1, slo:shi + 1].reshape(wsum.shape[0], -1)
    out = part.sum(axis=1, dtype=np.float32)
    exact = part.astype(np.int64).sum(axis=1)
    assert np.abs(part.astype(np.int64)).sum(axis=1).max(initial=0) < 2 ** 24 and np.array_equal(out.astype(np.int64), exact)
    return out


def zero_point_term(wsum, zp, H, W, stride, pad):
    """[P, Q, K] float32: per output pixel, the float32 sum of wsum[k, r, s] over the taps inside the image, then ONE
    float32 multiply by zp.  No class index."""
    K, R, S = wsum.shape
    P, Q = out_hw(H, W, R, S, stride, pad)
    out = np.empty((P, Q, K), np.float32)
    for p in range(P):
        rlo, rhi = window(p, R, H, stride, pad)
        for q in range(Q):
            slo, shi = window(q, S, W, stride, pad)
            out[p, q] = rect_sum(wsum, rlo, rhi, slo, shi) * np.float32(zp)
    return out


def epilogue(acc, b0, scale, bias, variant):
    """csrc/common.h epilogue_one, restated: v = f32(acc) - bias0; no bias: f16(v * scale); variant 0: f16(fma(v, scale,
    bias)); variant 1: f16(f32(v * scale) + bias).  Every operation one float32 rounding, then one to FP16."""
    v = acc.astype(np.float32) - b0.astype(np.float32)
    sc = np.broadcast_to(scale.astype(np.float32), v.shape)
    if bias is None:
        r = v * sc
    elif variant == 0:
        r = ei.fma32(v, sc, bias.astype(np.float32))
    else:
        r = (v * sc) + bias.astype(np.float32)
    assert r.dtype == np.float32
    with np.errstate(over="ignore"):
        return r.astype(np.float16)


def add_f16(a, b):
    """The residual add: f16(f32(a) + f32(b))."""
    return (a.astype(np.float32) + b.astype(np.float32)).astype(np.float16)


@functools.lru_cache(maxsize=None)
def _accumulators(key):
    c = dict(key)
    d = inputs(c)
    acc = ei.conv_accumulate(d["x"].transpose(0, 3, 1, 2), d["w"].transpose(0, 3, 1, 2), c["stride"], c["pad"],
                             dtype=np.int64)                              # [n, K, P, Q]
    assert np.abs(acc).max(initial=0) < 2 ** 31
    acc = np.ascontiguousarray(acc.transpose(0, 2, 3, 1)).astype(np.int32)  # [n, P, Q, K]
    acc.setflags(write=False)
    return acc


def accumulators(c):
    """Exact int64 accumulation (tests/exact_inputs.conv_accumulate), kept as int32 [n, P, Q, K]: computed once per
    case and shared."""
    return _accumulators(tuple(sorted(c.items())))


def wsum_of(w):
    """[K, R, S] float32 tap sums over the input channels (exact: |sum| <= 128 C)."""
    return w.astype(np.float32).sum(axis=3, dtype=np.float32)


def reference(c, variant, with_residual=True):
    """Expected FP16 output [n, P, Q, K] of an INT8 / W4 case under one epilogue variant."""
    d = inputs(c)
    acc = accumulators(c)
    b0 = zero_point_term(wsum_of(d["w"]), ZP, c["H"], c["W"], c["stride"], c["pad"])
    out = epilogue(acc, b0[None], d["scale"], d["bias"], variant)
    if with_residual and d["residual"] is not None:
        r = d["residual"]
        out = add_f16(out, r if c["residual"] == "full" else r[:, None, None, :])
    return out


def f16_case(c):
    """tests/exact_inputs.conv2d of an FP16 case (integer-valued operands: the result is exact in any order)."""
    return ei.conv2d(c["n"], c["C"], c["H"], c["W"], c["K"], (c["R"], c["S"]), c["stride"], c["pad"], c["bias"],
                     {"": None, "full": "full", "image": "per_image"}[c["residual"]])
