"""The workgroup -> tile map past one super-row (cases: tests/tile_map.py): one configuration per kernel family of the
GEMM / conv family on 9 and 11 m-tiles by 1 and 3 n-tiles -- a second super-row, a partial last one, XCD runs of
unequal length --, every halo tile on 9 and 18 pixel tiles, the GEMM + LayerNorm launch in both record forms, the
persistent kernel with one and with several tiles per workgroup.

Every result is compared bit for bit with the C oracle, on random operands and on index-coded ones whose exact result
names the tile it belongs to (tests/tile_map.py coded_*).  Outputs are written into 0x5A-filled buffers between guard
zones: a tile no workgroup computed keeps the fill, a write outside the output breaks a guard.

tests/test_env_switches_gpu.py runs the index-coded cases on 11 m-tiles again in child processes under
MIXDQ_IGEMM_GM = 1, 2 and 64 (the expectation does not depend on the order in which the tiles are computed)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import detdata as dd
from tests import exact_inputs as ei
from tests import tile_map as tm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, FILL = 256, 0x5A
KINDS = ("random", "coded")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scal(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def seed_of(c):
    s = 23
    for v in (c["cfg"], c["tiles_m"], c["tiles_n"], c.get("K", 0), len(c["family"])):
        s = (s * 1000003 + int(v)) % (1 << 31)
    return s


class Out:
    """A device output of `shape` between two guard zones, everything filled with 0x5A."""

    def __init__(self, shape, dtype):
        self.nb = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((GUARD + self.nb + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 256 == 0
        self.t = self.raw[GUARD:GUARD + self.nb].view(dtype).reshape(shape)
        assert self.t.is_contiguous() and self.t.data_ptr() == self.raw.data_ptr() + GUARD

    def numpy(self, what):
        torch.cuda.synchronize()
        r = self.raw.cpu().numpy()
        assert (r[:GUARD] == FILL).all() and (r[GUARD + self.nb:] == FILL).all(), f"{what}: a guard zone was written"
        return self.t.cpu().numpy()


def bits_equal(got, want, what, tile=None):
    g = got.view(np.uint16) if got.dtype == np.float16 else got
    w = want.view(np.uint16) if want.dtype == np.float16 else want
    assert g.shape == w.shape, f"{what}: shape {g.shape} vs {w.shape}"
    bad = np.argwhere(g != w)
    if bad.size:
        at = tuple(bad[0])
        where = "" if tile is None else f" (tile {tuple(int(i) // b for i, b in zip(at[-2:], tile))} of {tile})"
        raise AssertionError(f"{what}: {len(bad)}/{g.size} elements differ; first at {at}{where}: "
                             f"got {got[at]!r} want {want[at]!r}")


def _epilogue(s, N, kind, bias=True):
    """(bias0, scale, bias): random, or the identity epilogue of the coded operands."""
    if kind == "coded":
        return np.zeros(N, np.float32), np.ones(N, np.float32), None
    return dd.f32(s + 2, (N,), -500, 500), dd.f32(s + 3, (N,), 1e-4, 1e-3), dd.f16(s + 4, (N,), -1, 1) if bias else None


def _opt(a):
    return None if a is None else t(a)


def _coded_want(acc):
    want = acc.astype(np.float16)
    assert np.array_equal(want.astype(np.int64), acc)
    return want


GEMM_CASES = [c for c in tm.CASES if c["family"] in tm.GEMM_FAMILIES and c["family"] not in ("conv", "grouped", "f16")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", GEMM_CASES, ids=[tm.case_id(c) for c in GEMM_CASES])
def test_gemm_families_past_one_super_row(C, oracle, monkeypatch, case, kind):
    """plain Linear on both staging paths, packed W4 / W2, GEMM + GEGLU, quantize-in-prologue, the four-phase tile and
    its persistent form (at its default grid: one tile per workgroup, and capped to 8 workgroups: up to five)."""
    from mixdq_amd.nn.utils import pack_w2, pack_w4, unpack_w2
    fam, cfg, M, N, K, bm, bn = (case[k] for k in ("family", "cfg", "M", "N", "K", "BM", "BN"))
    s, v = seed_of(case), C.FLAGS & 1
    what = f"{tm.case_id(case)} {kind}"
    if kind == "coded":
        a, w, acc = (tm.coded_gemm_narrow if fam == "w2" else tm.coded_gemm)(M, N, K, bm, bn, s)
    else:
        lo, hi = {"w4": (-8, 8), "w2": (-2, 2)}.get(fam, (-128, 128))
        a, w = dd.int8(s, (M, K)), dd.int8(s + 1, (N, K), lo, hi)
    b0, sc, bias = _epilogue(s, N, kind, bias=case["tiles_m"] == 9)
    kw = {}
    wd = t(w)
    if fam == "w4":
        p = pack_w4(torch.from_numpy(w))
        assert np.array_equal(oracle.unpack_w4(p.numpy()), w)
        wd, kw = p.to(DEV), dict(_w4=True)
    elif fam == "w2":
        p = pack_w2(torch.from_numpy(w))
        assert torch.equal(unpack_w2(p), torch.from_numpy(w))
        wd, kw = p.to(DEV), dict(_w2=True)

    if fam == "geglu":
        if kind == "coded":
            sc = np.full(N, 0.125, np.float32)           # h = code / 8 <= 8: the product stays inside the quantizer
        s_inv, zp = (1.9, -128.0) if kind == "coded" else (float(np.float32(1) / np.float32(0.02)), -60.0)
        want = oracle.geglu_quantize(oracle.qlinear(a, w, b0, sc, bias, v), s_inv, zp, v)[0]
        if kind == "coded":
            assert want.min() > -128 and want.max() < 127 and len(np.unique(want)) >= 8
        perm = C.geglu_row_order(N // 2, DEV)
        out = Out((M, N // 2), torch.int8)
        C.qlinear_geglu(t(a), wd[perm].contiguous(), t(sc)[perm].contiguous(), t(b0)[perm].contiguous(),
                        None if bias is None else t(bias)[perm].contiguous(), scal(s_inv), scal(zp), _cfg=cfg, _out=out.t)
        bits_equal(out.numpy(what), want, what, (bm, bn // 2))
        return

    if fam == "f16in":
        if kind == "coded":
            x, s_inv, zp = a.astype(np.float16), 1.0, 0.0
        else:
            x, s_inv, zp = dd.f16(s, (M, K), -4, 4), 31.37, -9.0
        q = oracle.quantize(x, s_inv, zp, v)
        assert kind != "coded" or np.array_equal(q, a)
        want = oracle.qlinear(q, w, b0, sc, bias, v)
        out = Out((M, N), torch.float16)
        C.qlinear_f16in(t(x), scal(s_inv), scal(zp), wd, t(sc), t(b0), _opt(bias), _cfg=cfg, _out=out.t)
        bits_equal(out.numpy(what), want, what, (bm, bn))
        return

    want = oracle.qlinear(a, w, b0, sc, bias, v)
    if kind == "coded":
        bits_equal(want, _coded_want(acc), what + " (the oracle on the coded operands)")
    grids = [None]
    if fam == "pp71":
        tiles = case["tiles_m"] * case["tiles_n"]
        assert N % 8 == 0 and K % 128 == 0 and K >= 256            # pp_ok: the persistent kernel takes the launch
        assert tm.persistent_grid(tiles) >= tiles and tm.persistent_grid(tiles, cap=8) == 8
        assert tm.persistent_seq(0, 1, 8, tiles) is not None       # capped: workgroup 0 walks on to a second tile
        grids = [None, 8]
    for cap in grids:
        if cap is not None:
            monkeypatch.setenv("MIXDQ_IGEMM_PERSIST_WGS", str(cap))
        out = Out((M, N), torch.float16)
        C.qlinear_w8_a8_ohalf(t(a), wd, t(sc), scal(1), scal(0), t(b0), t(sc), t(b0), _opt(bias), _cfg=cfg, _out=out.t,
                              **kw)
        bits_equal(out.numpy(what), want, what + ("" if cap is None else f" on {cap} workgroups"), (bm, bn))


F16_CASES = [c for c in tm.CASES if c["family"] == "f16"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", F16_CASES, ids=[tm.case_id(c) for c in F16_CASES])
def test_f16_linear_past_one_super_row(C, case, kind):
    """Integer-valued FP16 operands (tests/exact_inputs.py): the FP32 accumulation is exact in any order."""
    cfg, M, N, K, bm, bn = (case[k] for k in ("cfg", "M", "N", "K", "BM", "BN"))
    what = f"{tm.case_id(case)} {kind}"
    if kind == "coded":
        a, w, acc = tm.coded_gemm(M, N, K, bm, bn, 5)
        x, wf, bias, want = a.astype(np.float16), w.astype(np.float16), None, _coded_want(acc)
    else:
        d = ei.linear(M, K, N, bias=True)
        x, wf, bias, want = d["x"], d["w"], d["bias"], d["expected"]
    out = Out((M, N), torch.float16)
    xd, wd, bd = t(x), t(wf), _opt(bias)
    code = C._lib.mixdq_linear_f16(xd.data_ptr(), wd.data_ptr(), None if bd is None else bd.data_ptr(),
                                   out.t.data_ptr(), M, N, K, None, 1, cfg << 8,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == 0, code
    bits_equal(out.numpy(what), want, what, (bm, bn))


GROUPED_CASES = [c for c in tm.CASES if c["family"] == "grouped"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", GROUPED_CASES, ids=[tm.case_id(c) for c in GROUPED_CASES])
def test_grouped_launch_past_one_super_row(C, oracle, case, kind):
    """Two members on one grid: each runs the map on ITS tile count (the narrow member's surplus workgroups leave)."""
    cfg, M, K, bm, bn = (case[k] for k in ("cfg", "M", "K", "BM", "BN"))
    s = seed_of(case)
    a = tm.coded_gemm(M, 4, K, bm, bn, s)[0] if kind == "coded" else dd.int8(s, (M, K))
    members, outs, wants = [], [], []
    for i, N in enumerate(case["Ns"]):
        if kind == "coded":
            _, w, acc = tm.coded_gemm(M, N, K, bm, bn, s + i)
            b0, sc, bias = np.full(N, -100.0 * i, np.float32), np.ones(N, np.float32), None      # + 100 i: the member
        else:
            w = dd.int8(s + 10 + i, (N, K))
            b0, sc, bias = _epilogue(s + 20 * i, N, kind, bias=i == 1)
        want = oracle.qlinear(a, w, b0, sc, bias, C.FLAGS & 1)
        if kind == "coded":
            bits_equal(want, _coded_want(acc + 100 * i), "the oracle on the coded operands")
        out = Out((M, N), torch.float16)
        outs.append(out)
        wants.append(want)
        members.append((t(w), t(b0), t(sc), _opt(bias), out.t))
    C.qlinear_grouped(t(a), C.GemmGroupTable(members), _cfg=cfg)
    for i, (out, want) in enumerate(zip(outs, wants)):
        what = f"{tm.case_id(case)} {kind} member {i}"
        bits_equal(out.numpy(what), want, what, (bm, bn))


# ----------------------------------------------------------------------------------------------------- convs
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _conv_call(C, x, w_dev, sc, wsum, zp, bias, n, H, W, Cin, K, flags, out):
    """mixdq_qconv2d_w8a8_table, 3x3 / stride 1 / pad 1, into `out` [n, H, W, K] (x: [n, H or H/2, W or W/2, Cin])."""
    xd, scd, bd, zpd = t(x), t(sc), _opt(bias), scal(zp)
    table = C.conv_border_table(t(wsum.reshape(K, 1, 3, 3)))
    code = C._lib.mixdq_qconv2d_w8a8_table(xd.data_ptr(), w_dev.data_ptr(), scd.data_ptr(), table.data_ptr(),
                                           zpd.data_ptr(), None, None if bd is None else bd.data_ptr(),
                                           out.t.data_ptr(), n, H, W, Cin, K, 3, 3, 1, 1, None, 1, C.FLAGS | flags,
                                           _stream())
    torch.cuda.synchronize()
    assert code == 0, f"status {code}"


def _conv_operands(C, oracle, case, kind, pixel_tile, n, H, W, Cin, K, bn, w4):
    from mixdq_amd.nn.utils import pack_w4
    s = seed_of(dict(case, K=K))
    if kind == "coded":
        x, w, acc = tm.coded_conv(n, H, W, Cin, K, pixel_tile, bn)
        sc, bias, zp = np.ones(K, np.float32), None, 0.0
    else:
        x = dd.int8(s, (n, H, W, Cin))
        w = dd.int8(s + 1, (K, 3, 3, Cin), *((-8, 8) if w4 else (-128, 128)))
        sc, bias, zp, acc = dd.f32(s + 2, (K,), 1e-4, 6e-4), dd.f16(s + 3, (K,), -1, 1), -11.0, None
    if w4:
        packed = pack_w4(torch.from_numpy(w))
        assert np.array_equal(oracle.unpack_w4(packed.numpy()), w)
        w_dev = packed.to(DEV)
    else:
        w_dev = t(w)
    wsum = w.astype(np.float32).sum(axis=3, dtype=np.float32)
    return x, w, w_dev, sc, wsum, zp, bias, acc


CONV_CASES = [c for c in tm.CASES if c["family"] == "conv"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CONV_CASES, ids=[tm.case_id(c) for c in CONV_CASES])
def test_implicit_gemm_conv_past_one_super_row(C, oracle, case, kind):
    cfg, H, W, Cin, bm, bn, K = (case[k] for k in ("cfg", "H", "W", "C", "BM", "BN", "N"))
    what = f"{tm.case_id(case)} {kind}"
    assert C.conv_halo_select(1, H, W, Cin, K, 3, 3, 1, 1) == 0
    pixel_tile = (np.arange(H * W) // bm).reshape(1, H, W)
    x, w, w_dev, sc, wsum, zp, bias, acc = _conv_operands(C, oracle, case, kind, pixel_tile, 1, H, W, Cin, K, bn, False)
    want = oracle.qconv2d(x, w, sc, wsum, zp, None, bias, 1, 1, C.FLAGS & 1)
    if kind == "coded":
        bits_equal(want, _coded_want(acc), what + " (the oracle on the coded operands)")
    out = Out((1, H, W, K), torch.float16)
    _conv_call(C, x, w_dev, sc, wsum, zp, bias, 1, H, W, Cin, K, cfg << 8, out)
    bits_equal(out.numpy(what).reshape(H * W, K), want.reshape(H * W, K), what, (bm, bn))


HALO_CASES = [c for c in tm.CASES if c["family"].startswith("halo")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", HALO_CASES, ids=[tm.case_id(c) for c in HALO_CASES])
def test_halo_conv_tiles_past_one_super_row(C, oracle, case, kind):
    """Every tile of MIXDQ_HALO_TILES, forced, on 3 x 3 whole pixel tiles per image and two channel tiles: 18 and 36
    workgroups, super-rows of 8 + 1 and 8 + 8 + 2 pixel tiles; the upsample fold; packed W4."""
    tile, n, H, W, Cin, K, th, tw, bn = (case[k] for k in ("cfg", "n", "H", "W", "C", "K", "TH", "TW", "BN"))
    what = f"{tm.case_id(case)} {kind}"
    assert C.conv_halo_select(n, H, W, Cin, K, 3, 3, 1, 1) != 0                 # inside the kernel's range
    tx = W // tw
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    per_image = (yy // th) * tx + xx // tw
    pixel_tile = np.stack([i * (H // th) * tx + per_image for i in range(n)])
    flags = tile << 8
    if case["ups"]:
        # the stored image is half the size: a source pixel feeds the 2 x 2 pixels of one tile (TH, TW even)
        src_tile = pixel_tile[:, ::2, ::2]
        assert np.array_equal(np.repeat(np.repeat(src_tile, 2, axis=1), 2, axis=2), pixel_tile)
        xs, w, w_dev, sc, wsum, zp, bias, acc = _conv_operands(C, oracle, case, kind, src_tile, n, H // 2, W // 2, Cin,
                                                               K, bn, False)
        x_full = np.repeat(np.repeat(xs, 2, axis=1), 2, axis=2)
        acc = None if acc is None else np.repeat(np.repeat(acc, 2, axis=1), 2, axis=2)
        x_in, flags = xs, flags | C.FLAG_UPSAMPLE2X
    else:
        x_full, w, w_dev, sc, wsum, zp, bias, acc = _conv_operands(C, oracle, case, kind, pixel_tile, n, H, W, Cin, K,
                                                                   bn, case["w4"])
        x_in = x_full
    if case["w4"]:
        flags |= C.FLAG_W4
    want = oracle.qconv2d(x_full, w, sc, wsum, zp, None, bias, 1, 1, C.FLAGS & 1)
    if kind == "coded":
        bits_equal(want, _coded_want(acc), what + " (the oracle on the coded operands)")
    out = Out((n, H, W, K), torch.float16)
    _conv_call(C, x_in, w_dev, sc, wsum, zp, bias, n, H, W, Cin, K, flags, out)
    got = out.numpy(what)
    bad = np.argwhere(got.view(np.uint16) != want.view(np.uint16))
    assert bad.size == 0, (f"{what}: {len(bad)}/{got.size} elements differ; first at (image, y, x, channel) "
                           f"{tuple(bad[0])}: pixel tile {pixel_tile[tuple(bad[0][:3])]}, channel tile {bad[0][3] // bn}: "
                           f"got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}")


# ------------------------------------------------------------------------------------------- GEMM + LayerNorm
LN_CASES = [c for c in tm.CASES if c["family"].startswith("ln_")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", LN_CASES, ids=[tm.case_id(c) for c in LN_CASES])
def test_gemm_layernorm_launch_both_record_forms(C, oracle, case, kind):
    """mixdq_qlinear_w8a8_ln on a forced tile: K = 256 takes the XCD-local records (row-major order behind the run
    formula), K = 2176 the global ones (the super-row map).  FP16 rows, one INT8 tensor and the FP16 LayerNorm copy
    against the oracle's chain; the workspace's sticky error word stays 0."""
    cfg, M, N, K, bm, bn = (case[k] for k in ("cfg", "M", "N", "K", "BM", "BN"))
    what = f"{tm.case_id(case)} {kind}"
    s, v = seed_of(case), C.FLAGS & 1
    if kind == "coded":
        a, w, acc = tm.coded_gemm(M, N, K, bm, bn, s)
        b0, sc, bias, res = np.zeros(N, np.float32), np.ones(N, np.float32), None, None
    else:
        a, w = dd.int8(s, (M, K)), dd.int8(s + 1, (N, K))
        b0, sc = dd.f32(s + 2, (N,), -500, 500), dd.f32(s + 3, (N,), 2e-5, 6e-5)
        bias, res = dd.f16(s + 4, (N,), -1, 1), dd.normal_f16(s + 5, (M, N), 1.5)
    gamma = (dd.normal_f16(s + 6, (N,), 0.3).astype(np.float32) + 1).astype(np.float16)
    beta = dd.normal_f16(s + 7, (N,), 0.2)
    qp = [(float(np.float32(1) / np.float32(0.02)), -7.0)]
    y_ref = oracle.qlinear(a, w, b0, sc, bias, v)
    if kind == "coded":
        bits_equal(y_ref, _coded_want(acc), what + " (the oracle on the coded operands)")
    if res is not None:
        y_ref = oracle.add_f16(y_ref, res)
    (q_ref,), h_ref = oracle.layernorm_quantize(y_ref, gamma, beta, 1e-5, qp, v)

    ws = C.qlinear_ln_workspace(M, N, DEV)
    y, q, h = Out((M, N), torch.float16), Out((M, N), torch.int8), Out((M, N), torch.float16)
    ad, wd, b0d, scd, bd, rd, gd, bed = t(a), t(w), t(b0), t(sc), _opt(bias), _opt(res), t(gamma), t(beta)
    si, zp = scal(qp[0][0]), scal(qp[0][1])
    arr = ctypes.c_void_p * 1
    code = C._lib.mixdq_qlinear_w8a8_ln(ad.data_ptr(), wd.data_ptr(), b0d.data_ptr(), scd.data_ptr(),
                                        None if bd is None else bd.data_ptr(), y.t.data_ptr(), M, N, K,
                                        None if rd is None else rd.data_ptr(), 1, gd.data_ptr(), bed.data_ptr(), 1e-5, 1,
                                        arr(si.data_ptr()), arr(zp.data_ptr()), arr(q.t.data_ptr()), h.t.data_ptr(),
                                        ws.data_ptr(), C.FLAGS | (cfg << 8), _stream())
    assert code == 0, f"status {code}"
    status = C.qlinear_ln_status(ws)
    assert status == 0, f"{what}: a workgroup gave up waiting for its row block's records (launch tag {status})"
    bits_equal(y.numpy(what), y_ref, what + " rows", (bm, bn))
    bits_equal(h.numpy(what), h_ref, what + " LayerNorm copy", (bm, bn))
    bits_equal(q.numpy(what), q_ref, what + " quantized", (bm, bn))
    assert ws[:8].view(torch.int32).tolist() == [1, 0]              # (epoch, departures): one launch, all gone
