"""The conv entry points over the geometry they accept (cases and reference: tests/conv_geometry.py), and every entry
point's behaviour with an operand off its 16- / 8-byte boundary.

Part 1: mixdq_qconv2d_w8a8[_table] (W8 and packed W4), mixdq_conv_border_table, mixdq_conv_zero_point_propagate and
mixdq_conv2d_f16 at R != S, pad > 1, stride 3, images smaller than the window -- equality of bits with a numpy
reference that computes the zero-point term by window intersection, never through a class index.

Part 2: offset operands.  The calls go through ctypes on the library handle mixdq_amd._C loads, not through the
Python wrappers: the wrappers re-align the float vectors (_f32vec) and allocate the outputs themselves, so only the
C entry lets a test give EVERY operand an offset and own the output with guard bytes on both sides.  Each operand in
turn gets the smallest offset that keeps its own element type naturally aligned (floats 4 bytes, halves 2, int8 1, 4
and 8); nothing is null or out of bounds.  The generic kernels must give the aligned call's bits; the packed and fused
entries must return their documented status (include/mixdq_hip.h) and write nothing.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_geometry as cg
from tests import detdata as dd
from tests import exact_inputs as ei

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, ERR_ALIGNMENT, ERR_W4, ERR_GEGLU, ERR_PADDING, ERR_SHAPE, ERR_W2 = 0, 2, 5, 6, 7, 9, 10


@pytest.fixture(params=["A", "B"], ids=["fma", "mul_add"])
def epilogue_variant(request, monkeypatch):
    """Both roundings of the epilogue's multiply-add (tests/test_halo_w4_gpu.py's pattern)."""
    import mixdq_amd._C as C_
    monkeypatch.setattr(C_, "FLAGS", 1 if request.param == "B" else 0)
    return request.param


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scal(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def nhwc(a):
    """[n, H, W, C] numpy -> the [n, C, H, W] channels-last tensor the wrappers take."""
    return t(a).permute(0, 3, 1, 2)


def assert_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
    gi, wi = g.view(f"u{g.itemsize}"), w.view(f"u{w.itemsize}")
    if not np.array_equal(gi, wi):
        bad = np.argwhere(gi != wi)
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ; first at {i}: got {g[i]!r} want {w[i]!r}")


# =============================================================================================== part 1: geometry
def _launch(C, c, d, w_dev, cfg, w4=False):
    """One INT8 conv launch of a case; returns [n, P, Q, K] numpy."""
    wsum = cg.wsum_of(d["w"])
    K, R, S, pad = c["K"], c["R"], c["S"], c["pad"]
    bias0 = cg.zero_point_term(wsum, cg.ZP, c["H"], c["W"], c["stride"], pad)[0, 0] if pad == 0 else None
    kw = {}
    if c["residual"] == "full":
        kw = dict(_residual=nhwc(d["residual"]))
    elif c["residual"] == "image":
        kw = dict(_residual=t(d["residual"]), _residual_per_image=True)
    sc = t(d["scale"])
    out = C.qconv2d_w8_a8_ohalf(nhwc(d["x"]), w_dev, sc, scal(1), scal(cg.ZP), sc,
                                t(wsum.reshape(K, 1, R, S)) if pad else None, t(bias0), t(d["bias"]), c["stride"], pad,
                                _cfg=cfg, _w4=w4, **kw)
    assert tuple(out.shape) == (c["n"], K, c["P"], c["Q"])
    return out.permute(0, 2, 3, 1).contiguous().cpu().numpy()


@pytest.mark.parametrize("case", cg.INT8_CASES, ids=[cg.case_id(c) for c in cg.INT8_CASES])
def test_qconv2d_w8a8_geometry(C, epilogue_variant, case):
    """Forced tile == the numpy reference == the automatic choice, bit for bit; C = 4 / 20 run the generic kernel."""
    d = cg.inputs(case)
    want = cg.reference(case, C.FLAGS & 1)
    got = _launch(C, case, d, nhwc(d["w"]), case["cfg"])
    assert_bits(got, want, cg.case_id(case))
    assert_bits(_launch(C, case, d, nhwc(d["w"]), 0), got, "automatic choice vs forced tile")
    sel = C.igemm_select_id(case["n"] * case["P"] * case["Q"], case["K"], case["C"], case["R"] * case["S"] * case["C"])
    assert (sel == 0) == (case["C"] in cg.C_GENERIC), f"select_id {sel}"
    assert C.conv_halo_select(case["n"], case["H"], case["W"], case["C"], case["K"], case["R"], case["S"],
                              case["stride"], case["pad"]) == 0


@pytest.mark.parametrize("case", cg.W4_CASES, ids=[cg.case_id(c) for c in cg.W4_CASES])
def test_qconv2d_w4_geometry(C, oracle, epilogue_variant, case):
    """Packed W4 on the implicit-GEMM family == the reference on the unpacked integers == the W8 launch on them."""
    from mixdq_amd.nn.utils import pack_w4
    d = cg.inputs(case)
    assert d["w"].min() == -8 and d["w"].max() == 7
    packed = pack_w4(torch.from_numpy(d["w"]))                       # [K, R, S, C / 2]
    assert np.array_equal(oracle.unpack_w4(packed.numpy()), d["w"])
    got = _launch(C, case, d, packed.to(DEV).permute(0, 3, 1, 2), case["cfg"], w4=True)
    assert_bits(got, cg.reference(case, C.FLAGS & 1), cg.case_id(case))
    assert_bits(_launch(C, case, d, nhwc(d["w"]), case["cfg"]), got, "W8 launch on the unpacked weights vs W4")


def _tap_sums(K, R, S, seed):
    return dd.int8(seed, (K, R, S), -128, 128).astype(np.float32) * np.float32(37)      # integers, |sum| < 2^24


@pytest.mark.parametrize("R,S", cg.RS, ids=[f"{r}x{s}" for r, s in cg.RS])
def test_border_table_rows_are_the_rectangle_sums(C, R, S):
    """Row ((rlo R + rhi) S + slo) S + shi of mixdq_conv_border_table == the sum of wsum[k, rlo..rhi, slo..shi], for
    every non-empty rectangle of all R R S S rows.

    Rows with rlo > rhi or slo > shi (empty rectangles) may hold anything (the kernel leaves 0 there): no launch reads
    them.  The rule: the class of an output pixel is its window's intersection with the image, rlo = max(0, -hb),
    rhi = min(R - 1, H - 1 - hb) with hb = p stride - pad in [-pad, H - 1 + pad - R + 1]; the INT8 entries refuse
    pad >= R and pad >= S (MIXDQ_ERR_PADDING), and with pad < R every window holds an image row: -hb <= pad <= R - 1
    gives rlo <= R - 1, hb <= H - 1 gives rhi >= 0, and rlo <= rhi because row max(0, hb) lies in both ranges.  The
    kernels' max(.., 0) / min(.., R - 1) clamps are therefore never active.  tests/test_conv_geometry_host.py checks
    that every class met by every case is a non-empty rectangle."""
    K = 12
    wsum = _tap_sums(K, R, S, 4100 + 16 * R + S)
    table = C.conv_border_table(t(wsum.reshape(K, 1, R, S))).cpu().numpy()
    assert table.shape == (R * R * S * S, K)
    seen = 0
    for rlo in range(R):
        for rhi in range(rlo, R):
            for slo in range(S):
                for shi in range(slo, S):
                    row = cg.class_index(R, S, rlo, rhi, slo, shi)
                    assert_bits(table[row], cg.rect_sum(wsum, rlo, rhi, slo, shi), f"class ({rlo},{rhi},{slo},{shi})")
                    seen += 1
    assert seen == (R * (R + 1) // 2) * (S * (S + 1) // 2)


@pytest.mark.parametrize("g", cg.GEOMETRIES, ids=str)
def test_zero_point_propagate_geometry(C, g):
    R, S, stride, pad = g
    K = 12
    wsum = _tap_sums(K, R, S, 4200 + 16 * R + S)
    for _, n, H, W in cg.images(*g):
        got = C.conv_zero_point_propagate(t(wsum.reshape(K, 1, R, S)), scal(cg.ZP), n, H, W, stride, pad)
        want = cg.zero_point_term(wsum, cg.ZP, H, W, stride, pad)
        assert_bits(got.permute(0, 2, 3, 1).contiguous(), np.broadcast_to(want[None], (n,) + want.shape), f"{g} {H}x{W}")


@pytest.mark.parametrize("case", cg.F16_CASES, ids=[cg.case_id(c) for c in cg.F16_CASES])
def test_conv2d_f16_geometry_exact(C, case):
    """Integer-valued operands: fp16(acc + bias), then the rounding of the residual add, and nothing else -- on the
    forced FP16 tile, on the automatic choice and (C % 8 != 0) on the generic kernel; pad >= R included."""
    e = cg.f16_case(case)
    x = t(e["x"]).contiguous(memory_format=torch.channels_last)
    kw = {}
    if case["residual"] == "full":
        kw = dict(_residual=t(e["residual"]).contiguous(memory_format=torch.channels_last))
    elif case["residual"] == "image":
        kw = dict(_residual=t(e["residual"]), _residual_per_image=True)
    for cfg in {case["cfg"], 0}:
        out = C.conv2d_f16(x, t(e["w"]), t(e["bias"]), case["stride"], case["pad"], _cfg=cfg, **kw)
        assert_bits(out.contiguous(), e["expected"], f"{cg.case_id(case)} cfg {cfg}")


@pytest.mark.parametrize("cfg", cg.TILES_F16)
def test_conv2d_f16_non_finite_pixel_stays_inside_its_windows(C, cfg):
    """One pixel of the input is +Inf in every channel: the outputs whose window does not hold it must keep their
    exact bits.  This is what the gather's `a_r < R` stop is for: K = R S C is no whole number of K-tiles here (144
    bytes against 64- and 128-byte tiles), and the chunks of the last K-tile past K would otherwise stage the image
    row BELOW the window; the weight tile holds zeros there, so INT8 accumulators cannot tell (x * 0 == 0: for the
    INT8 kernels the stop is redundant), but Inf * 0 is NaN."""
    n, Cin, H, W, K, R, S, stride, pad = 1, 8, 9, 7, 12, 3, 3, 1, 1
    e = ei.conv2d(n, Cin, H, W, K, (R, S), stride, pad, True)
    hot = (5, 3)
    x = e["x"].copy()
    x[0, :, hot[0], hot[1]] = np.inf
    out = C.conv2d_f16(t(x).contiguous(memory_format=torch.channels_last), t(e["w"]), t(e["bias"]), stride, pad, _cfg=cfg)
    got = out.contiguous().cpu().numpy()                                  # [n, K, P, Q]
    p, q = np.meshgrid(np.arange(got.shape[2]), np.arange(got.shape[3]), indexing="ij")
    sees = (np.abs(p - hot[0]) <= 1) & (np.abs(q - hot[1]) <= 1)        # 3x3 / stride 1 / pad 1: window centre (p, q)
    assert sees.sum() == 9
    assert_bits(got[:, :, ~sees], e["expected"][:, :, ~sees], f"cfg {cfg}: outputs whose window misses the pixel")


def _halo_args(R, S, pad, K=80, Cin=64):
    v = torch.ones(K, device=DEV)
    ws = torch.ones(K, 1, R, S, device=DEV)
    w = torch.zeros(K, R, S, Cin, dtype=torch.int8, device=DEV).permute(0, 3, 1, 2)
    return w, (v, scal(1), scal(0), v, ws if pad else None, None if pad else v, None)


@pytest.mark.parametrize("g", cg.GEOMETRIES[:-1], ids=str)
def test_halo_kernel_range_excludes_every_other_geometry(C, g):
    """Only 3x3 / stride 1 / pad 1 runs on the LDS-halo kernel: the query answers 0, a forced halo tile and the
    upsample fold are refused (MIXDQ_ERR_SHAPE), on an image the control geometry does run on."""
    R, S, stride, pad = g
    assert C.conv_halo_select(1, 16, 16, 64, 80, 3, 3, 1, 1) != 0
    for w4 in (False, True):
        assert C.conv_halo_select(1, 16, 16, 64, 80, R, S, stride, pad, w4=w4) == 0
    w, args = _halo_args(R, S, pad)
    x = torch.zeros(1, 16, 16, 64, dtype=torch.int8, device=DEV).permute(0, 3, 1, 2)
    for cfg in (90, 91, 92, 93):
        with pytest.raises(RuntimeError, match="shape outside"):
            C.qconv2d_w8_a8_ohalf(x, w, *args, stride, pad, _cfg=cfg)
    small = torch.zeros(1, 8, 8, 64, dtype=torch.int8, device=DEV).permute(0, 3, 1, 2)
    assert not C.conv_upsample2x_supported(tuple(small.shape), (80, 64, R, S), stride, pad)
    with pytest.raises(RuntimeError, match="shape outside"):
        C.qconv2d_w8_a8_ohalf(small, w, *args, stride, pad, _upsample2x=True)


# =============================================================================================== part 2: raw calls
GUARD, FILL, SENTINEL = 64, 0xA5, 0x5A


class Buf:
    """Device bytes [guard | offset | payload | guard]: the payload starts `off` bytes past a 256-byte boundary."""

    def __init__(self, arr, off=0, sentinel=False):
        a = np.ascontiguousarray(arr)
        assert off % min(a.itemsize, 16) == 0, "an operand is never placed off its element's natural alignment"
        self.dtype, self.shape, self.nb, self.lo = a.dtype, a.shape, a.nbytes, GUARD + off
        self.raw = torch.full((GUARD + 16 + a.nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 256 == 0 and off < 16
        self.raw[self.lo:self.lo + self.nb] = SENTINEL if sentinel else t(a.reshape(-1).view(np.uint8))
        self.ptr = self.raw.data_ptr() + self.lo

    def value(self):
        return self.raw[self.lo:self.lo + self.nb].cpu().numpy().view(self.dtype).reshape(self.shape)

    def untouched(self):
        """Guards intact -- and, for a sentinel-filled output, the payload too."""
        r = self.raw.cpu().numpy()
        return bool((r[:self.lo] == FILL).all() and (r[self.lo + self.nb:] == FILL).all())

    def still_sentinel(self):
        return self.untouched() and bool((self.raw[self.lo:self.lo + self.nb] == SENTINEL).all())


def _bufs(arrays, offsets, out_name="D"):
    return {k: (None if a is None else Buf(a, offsets.get(k, 0), sentinel=k == out_name)) for k, a in arrays.items()}


def _p(b):
    return None if b is None else ctypes.c_void_p(b.ptr)


def _sync_status(code):
    torch.cuda.synchronize()
    return int(code)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _offsets(names_int8, names_f32, names_f16):
    return ([(n, o) for n in names_int8 for o in (1, 4, 8)] + [(n, 4) for n in names_f32] + [(n, 2) for n in names_f16])


def _linear_arrays(M, N, K, seed):
    return dict(A=dd.int8(seed, (M, K)), W=dd.int8(seed + 1, (N, K)), bias0=dd.f32(seed + 2, (N,), -300, 300),
                scale=dd.f32(seed + 3, (N,), 1e-4, 1e-3), bias=dd.f16(seed + 4, (N,), -1, 1),
                D=np.zeros((M, N), np.float16), residual=dd.normal_f16(seed + 5, (M, N), 2.0))


def _rows_call(C, b, M, N, K, rm=(0, 0, 0), residual=True, flags=0):
    code = C._lib.mixdq_qlinear_w8a8_rows(_p(b["A"]), _p(b["W"]), _p(b["bias0"]), _p(b["scale"]), _p(b["bias"]),
                                          _p(b["D"]), M, N, K, *rm, _p(b["residual"]) if residual else None, 1,
                                          C.FLAGS | flags, _stream())
    return _sync_status(code)


def test_offset_operands_qlinear_rows(C, oracle, epilogue_variant):
    """Every operand of mixdq_qlinear_w8a8_rows off its boundary in turn: the generic kernel gives the aligned call's
    bits (== the oracle) and writes nothing outside D; once with an output row map."""
    M, N, K = 37, 24, 64
    arrs = _linear_arrays(M, N, K, 5100)
    b = _bufs(arrs, {})
    assert _rows_call(C, b, M, N, K) == OK and b["D"].untouched()
    base = b["D"].value()
    want = oracle.add_f16(oracle.qlinear(arrs["A"], arrs["W"], arrs["bias0"], arrs["scale"], arrs["bias"], C.FLAGS & 1),
                          arrs["residual"])
    assert_bits(base, want, "aligned call vs oracle")
    for name, off in _offsets(("A", "W"), ("bias0", "scale"), ("bias", "D", "residual")):
        b = _bufs(arrs, {name: off})
        assert b[name].ptr % 16 == off
        assert _rows_call(C, b, M, N, K) == OK, f"{name} + {off}"
        assert b["D"].untouched(), f"{name} + {off}: bytes outside D were written"
        assert_bits(b["D"].value(), base, f"{name} + {off}")
    # row map: 1 group row skipped in front of each group of rows; the residual cannot ride with a row map
    g, rows = 1, M
    arrs_rm = dict(arrs, D=np.zeros((g, rows + 1, N), np.float16))
    plain = oracle.qlinear(arrs["A"], arrs["W"], arrs["bias0"], arrs["scale"], arrs["bias"], C.FLAGS & 1)
    for offs in ({}, {"A": 1}, {"D": 2}):
        b = _bufs(arrs_rm, offs)
        assert _rows_call(C, b, M, N, K, rm=(rows, rows + 1, 1), residual=False) == OK and b["D"].untouched()
        d = b["D"].value()
        assert_bits(d[:, 1:].reshape(M, N), plain, f"row map {offs}")
        assert (d[:, 0].view(np.uint8) == SENTINEL).all(), "a row outside the map was written"


def _conv_arrays(n, H, W, Cin, K, R, S, stride, pad, seed):
    P, Q = cg.out_hw(H, W, R, S, stride, pad)
    w = dd.int8(seed + 1, (K, R, S, Cin))
    wsum = cg.wsum_of(w)
    table = np.zeros((R * R * S * S, K), np.float32)
    for rlo in range(R):
        for rhi in range(rlo, R):
            for slo in range(S):
                for shi in range(slo, S):
                    table[cg.class_index(R, S, rlo, rhi, slo, shi)] = cg.rect_sum(wsum, rlo, rhi, slo, shi)
    bias0 = cg.rect_sum(wsum, 0, R - 1, 0, S - 1) * np.float32(cg.ZP)
    return dict(X=dd.int8(seed, (n, H, W, Cin)), Wt=w, scale=dd.f32(seed + 2, (K,), 1e-4, 6e-4),
                table=table if pad else None, zp=np.asarray([cg.ZP], np.float32), bias0=None if pad else bias0,
                bias=dd.f16(seed + 3, (K,), -1, 1), D=np.zeros((n, P, Q, K), np.float16),
                residual=dd.normal_f16(seed + 4, (n, P, Q, K), 2.0)), wsum


def _table_call(C, b, n, H, W, Cin, K, R, S, stride, pad, flags=0):
    code = C._lib.mixdq_qconv2d_w8a8_table(_p(b["X"]), _p(b["Wt"]), _p(b["scale"]), _p(b["table"]), _p(b["zp"]),
                                           _p(b["bias0"]), _p(b["bias"]), _p(b["D"]), n, H, W, Cin, K, R, S, stride, pad,
                                           _p(b["residual"]), 1, C.FLAGS | flags, _stream())
    return _sync_status(code)


@pytest.mark.parametrize("pad", [0, 1])
def test_offset_operands_qconv2d_table(C, oracle, epilogue_variant, pad):
    geo = (2, 6, 5, 16, 12, 3, 3, 1, pad)
    arrs, wsum = _conv_arrays(*geo, seed=5200 + pad)
    b = _bufs(arrs, {})
    assert _table_call(C, b, *geo) == OK and b["D"].untouched()
    base = b["D"].value()
    want = oracle.qconv2d(arrs["X"], arrs["Wt"], arrs["scale"], wsum if pad else None, cg.ZP, arrs["bias0"],
                          arrs["bias"], 1, pad, C.FLAGS & 1)
    assert_bits(base, oracle.add_f16(want, arrs["residual"]), "aligned call vs oracle")
    for name, off in _offsets(("X", "Wt"), ("scale", "table" if pad else "bias0"), ("bias", "D", "residual")):
        b = _bufs(arrs, {name: off})
        assert _table_call(C, b, *geo) == OK, f"{name} + {off}"
        assert b["D"].untouched(), f"{name} + {off}: bytes outside D were written"
        assert_bits(b["D"].value(), base, f"{name} + {off}")


def test_offset_operand_takes_a_halo_shape_to_the_generic_kernel(C, epilogue_variant):
    """1 x 8 x 8 x 64 -> 80, 3x3 / 1 / 1 runs on the LDS-halo kernel; with X one byte off it must fall through to the
    generic kernel and give the same bits; a forced halo tile and the upsample fold are then refused."""
    geo = (1, 8, 8, 64, 80, 3, 3, 1, 1)
    assert C.conv_halo_select(*geo) != 0
    arrs, _ = _conv_arrays(*geo, seed=5300)
    b = _bufs(arrs, {})
    assert _table_call(C, b, *geo) == OK and b["D"].untouched()
    base = b["D"].value()
    for name, off in (("X", 1), ("table", 4), ("D", 2), ("bias", 2)):
        b = _bufs(arrs, {name: off})
        assert _table_call(C, b, *geo) == OK and b["D"].untouched(), f"{name} + {off}"
        assert_bits(b["D"].value(), base, f"{name} + {off}")
        assert _table_call(C, _bufs(arrs, {name: off}), *geo, flags=91 << 8) == ERR_SHAPE
    # MIXDQ_FLAG_UPSAMPLE2X: X is the 4 x 4 tensor, H and W the upsampled 8 x 8
    small = dict(arrs, X=arrs["X"][:, :4, :4].copy())
    ok = _bufs(small, {})
    assert _table_call(C, ok, *geo, flags=C.FLAG_UPSAMPLE2X) == OK and not ok["D"].still_sentinel()
    for name, off in (("X", 1), ("Wt", 8), ("scale", 4), ("residual", 2)):
        b = _bufs(small, {name: off})
        assert _table_call(C, b, *geo, flags=C.FLAG_UPSAMPLE2X) == ERR_SHAPE, f"{name} + {off}"
        assert b["D"].still_sentinel()


def test_offset_operands_linear_f16(C):
    M, K, N = 9, 24, 12
    e = ei.linear(M, K, N, True, True)
    arrs = dict(A=e["x"], W=e["w"], bias=e["bias"], D=np.zeros((M, N), np.float16), residual=e["residual"])
    for name, off in [("", 0)] + _offsets((), (), ("A", "W", "bias", "D", "residual")):
        b = _bufs(arrs, {name: off})
        code = C._lib.mixdq_linear_f16(_p(b["A"]), _p(b["W"]), _p(b["bias"]), _p(b["D"]), M, N, K, _p(b["residual"]), 1, 0,
                                       _stream())
        assert _sync_status(code) == OK and b["D"].untouched(), f"{name} + {off}"
        assert_bits(b["D"].value(), e["expected"], f"{name} + {off}")


def test_offset_operands_conv2d_f16(C):
    n, Cin, H, W, K, R, S, stride, pad = 2, 8, 5, 4, 12, 3, 2, 1, 1
    e = ei.conv2d(n, Cin, H, W, K, (R, S), stride, pad, True, "full")
    to_nhwc = lambda a: np.ascontiguousarray(a.transpose(0, 2, 3, 1))
    arrs = dict(X=to_nhwc(e["x"]), W=to_nhwc(e["w"]), bias=e["bias"], D=np.zeros(to_nhwc(e["expected"]).shape, np.float16),
                residual=to_nhwc(e["residual"]))
    for name, off in [("", 0)] + _offsets((), (), ("X", "W", "bias", "D", "residual")):
        b = _bufs(arrs, {name: off})
        code = C._lib.mixdq_conv2d_f16(_p(b["X"]), _p(b["W"]), _p(b["bias"]), _p(b["D"]), n, H, W, Cin, K, R, S, stride, pad,
                                       _p(b["residual"]), 1, 0, _stream())
        assert _sync_status(code) == OK and b["D"].untouched(), f"{name} + {off}"
        assert_bits(b["D"].value(), to_nhwc(e["expected"]), f"{name} + {off}")


@pytest.mark.parametrize("g", cg.REFUSED, ids=str)
def test_int8_entries_refuse_padding_not_below_the_kernel_size(C, g):
    """MIXDQ_ERR_PADDING from both INT8 conv entries, nothing written; the Python wrapper raises."""
    R, S, stride, pad = g
    geo = (1, 6, 5, 16, 12, R, S, stride, pad)
    arrs, wsum = _conv_arrays(*geo, seed=5400)
    b = _bufs(dict(arrs, table=np.zeros((R * R * S * S, 12), np.float32)), {})
    assert _table_call(C, b, *geo) == ERR_PADDING and b["D"].still_sentinel()
    ws, wk = Buf(wsum), Buf(np.zeros((R * R * S * S, 12), np.float32))
    code = C._lib.mixdq_qconv2d_w8a8(_p(b["X"]), _p(b["Wt"]), _p(b["scale"]), _p(ws), _p(b["zp"]), None, _p(b["bias"]),
                                     _p(b["D"]), _p(wk), 1, 6, 5, 16, 12, R, S, stride, pad, 1, C.FLAGS, _stream())
    assert _sync_status(code) == ERR_PADDING and b["D"].still_sentinel()
    v = torch.ones(12, device=DEV)
    with pytest.raises(RuntimeError, match="padding must be smaller"):
        C.qconv2d_w8_a8_ohalf(nhwc(arrs["X"]), nhwc(arrs["Wt"]), v, scal(1), scal(cg.ZP), v,
                              t(wsum.reshape(12, 1, R, S)), None, None, stride, pad)


def test_offset_operands_refused_by_the_packed_and_fused_gemm_entries(C):
    """W4 / W2 (MIXDQ_ERR_W4_SHAPE / _W2_SHAPE), GEMM + GEGLU (_GEGLU_SHAPE), the grouped launch's A, to_q +
    attention, GEMM + LayerNorm (_ALIGNMENT) and the quantizing GEMM (_SHAPE): the status, and a sentinel-filled
    output left as it was."""
    M, N, K = 37, 32, 64
    arrs = _linear_arrays(M, N, K, 5500)
    for flag, div, status in ((C.FLAG_W4, 2, ERR_W4), (C.FLAG_W2, 4, ERR_W2)):
        packed = dict(arrs, W=arrs["W"][:, :K // div].copy())
        for name, off in (("A", 1), ("W", 8), ("scale", 4), ("bias0", 4), ("bias", 2), ("D", 2), ("residual", 2)):
            b = _bufs(packed, {name: off})
            assert _rows_call(C, b, M, N, K, flags=flag) == status, f"flag {flag}: {name} + {off}"
            assert b["D"].still_sentinel()
    # GEMM + GEGLU: out int8 [M, N / 2]
    g = dict(arrs, D=np.zeros((M, N // 2), np.int8), sinv=np.asarray([50.0], np.float32), zp=np.asarray([3.0], np.float32))
    for name, off in (("A", 1), ("W", 4), ("scale", 4), ("bias0", 4), ("bias", 2), ("D", 4)):
        b = _bufs(g, {name: off})
        code = C._lib.mixdq_qlinear_w8a8_geglu(_p(b["A"]), _p(b["W"]), _p(b["bias0"]), _p(b["scale"]), _p(b["bias"]),
                                               _p(b["D"]), M, N, K, _p(b["sinv"]), _p(b["zp"]), C.FLAGS, _stream())
        assert _sync_status(code) == ERR_GEGLU and b["D"].still_sentinel(), f"geglu: {name} + {off}"
    # grouped: the shared A (the members' own operands are checked where the table is built)
    out = torch.full((M, N), 7.0, dtype=torch.float16, device=DEV)
    table = C.GemmGroupTable([(t(arrs["W"]), t(arrs["bias0"]), t(arrs["scale"]), None, out)])
    for off in (1, 4, 8):
        a = Buf(arrs["A"], off)
        code = C._lib.mixdq_qlinear_w8a8_grouped(_p(a), table.table.data_ptr(), 1, M, N, K, 0, 0, 0, C.FLAGS, _stream())
        assert _sync_status(code) == ERR_ALIGNMENT and bool((out == 7.0).all()), f"grouped: A + {off}"
    # to_q + cross-attention: M = T = 64 rows, N = K = 128, 77 keys
    Ma, Na, Tk = 64, 128, 77
    at = dict(A=dd.int8(5600, (Ma, Na)), W=dd.int8(5601, (Na, Na)), bias0=dd.f32(5602, (Na,), -30, 30),
              scale=dd.f32(5603, (Na,), 1e-4, 6e-4), k=dd.normal_f16(5604, (Tk, Na), 1.0),
              v=dd.normal_f16(5605, (Tk, Na), 1.0), D=np.zeros((Ma, Na), np.float16))
    for name, off in (("A", 1), ("W", 4), ("bias0", 4), ("scale", 4), ("k", 2), ("v", 2), ("D", 2)):
        b = _bufs(at, {name: off})
        code = C._lib.mixdq_qlinear_w8a8_attn(_p(b["A"]), _p(b["W"]), _p(b["bias0"]), _p(b["scale"]), _p(b["k"]), _p(b["v"]),
                                              _p(b["D"]), Ma, Na, Na, Ma, Tk, Tk * Na, Na, Tk * Na, Na, 0.125, None, None,
                                              C.FLAGS, _stream())
        assert _sync_status(code) == ERR_ALIGNMENT and b["D"].still_sentinel(), f"attn: {name} + {off}"
    # GEMM + residual + LayerNorm + quantize: 128 x 640 x 640
    Ml, Nl = 128, 640
    assert C.qlinear_ln_supported(Ml, Nl, Nl)
    ln = dict(A=dd.int8(5700, (Ml, Nl)), W=dd.int8(5701, (Nl, Nl)), bias0=dd.f32(5702, (Nl,), -50, 50),
              scale=dd.f32(5703, (Nl,), 2e-5, 6e-5), bias=dd.f16(5704, (Nl,), -1, 1), D=np.zeros((Ml, Nl), np.float16),
              residual=dd.normal_f16(5705, (Ml, Nl), 1.0), gamma=dd.f16(5706, (Nl,), 0.5, 1.5), beta=dd.f16(5707, (Nl,), -1, 1))
    ws = C.qlinear_ln_workspace(Ml, Nl, DEV)
    q = torch.full((Ml, Nl), 0x5A, dtype=torch.int8, device=DEV)
    sinv, zp = scal(25.0), scal(-3.0)
    arr = ctypes.c_void_p * 1
    for name, off in (("A", 1), ("W", 8), ("bias0", 4), ("scale", 4), ("bias", 2), ("D", 2), ("residual", 2), ("gamma", 2),
                      ("beta", 2)):
        b = _bufs(ln, {name: off})
        code = C._lib.mixdq_qlinear_w8a8_ln(_p(b["A"]), _p(b["W"]), _p(b["bias0"]), _p(b["scale"]), _p(b["bias"]), _p(b["D"]),
                                            Ml, Nl, Nl, _p(b["residual"]), 1, _p(b["gamma"]), _p(b["beta"]), 1e-5, 1,
                                            arr(sinv.data_ptr()), arr(zp.data_ptr()), arr(q.data_ptr()), None,
                                            ws.data_ptr(), C.FLAGS, _stream())
        assert _sync_status(code) == ERR_ALIGNMENT and b["D"].still_sentinel() and bool((q == 0x5A).all()), f"ln: {name} + {off}"
    assert not ws.any(), "a refused launch touched the workspace"
    # the quantizing GEMM
    Mf, Nf, Kf = 128, 640, 640
    fi = dict(A=dd.normal_f16(5800, (Mf, Kf), 1.0), W=dd.int8(5801, (Nf, Kf)), bias0=dd.f32(5802, (Nf,), -30, 30),
              scale=dd.f32(5803, (Nf,), 1e-4, 6e-4), bias=dd.f16(5804, (Nf,), -1, 1), D=np.zeros((Mf, Nf), np.float16),
              residual=dd.normal_f16(5805, (Mf, Nf), 1.0))
    assert C._lib.mixdq_qlinear_f16in_supported(Mf, Nf, Kf, Kf, Mf, 0)
    for name, off in [("", 0), ("A", 2), ("W", 1), ("bias0", 4), ("scale", 4), ("bias", 2), ("D", 2), ("residual", 2)]:
        b = _bufs(fi, {name: off})
        code = C._lib.mixdq_qlinear_f16in_w8a8(_p(b["A"]), Kf, sinv.data_ptr(), zp.data_ptr(), _p(b["W"]), _p(b["bias0"]),
                                               _p(b["scale"]), _p(b["bias"]), _p(b["D"]), Mf, Nf, Kf, 0, 0, 0,
                                               _p(b["residual"]), 1, C.FLAGS, _stream())
        if not name:
            assert _sync_status(code) == OK and b["D"].untouched() and not b["D"].still_sentinel()
        else:
            assert _sync_status(code) == ERR_SHAPE and b["D"].still_sentinel(), f"f16in: {name} + {off}"


def test_offset_operands_refused_by_attention_and_the_sampler_step(C):
    B, heads, D, T = 1, 1, 64, 8
    at = dict(q=dd.normal_f16(5900, (T, D), 1.0), k=dd.normal_f16(5901, (T, D), 1.0), v=dd.normal_f16(5902, (T, D), 1.0),
              D=np.zeros((T, D), np.float16))
    for name, off in [("", 0), ("q", 2), ("k", 2), ("v", 2), ("D", 2)]:
        b = _bufs(at, {name: off})
        code = C._lib.mixdq_attention_f16(_p(b["q"]), _p(b["k"]), _p(b["v"]), _p(b["D"]), B, heads, D, T, T,
                                          T * D, D, T * D, D, T * D, D, T * D, D, 0.125, None, None, C.FLAGS, _stream())
        if not name:
            assert _sync_status(code) == OK and b["D"].untouched() and not b["D"].still_sentinel()
        else:
            assert _sync_status(code) == ERR_ALIGNMENT and b["D"].still_sentinel(), f"attention: {name} + {off}"
    # sampler step: x (fp32 state, updated in place), eps / in fp16, coef [n_steps, 4], noise
    n, steps = 64, 2
    x0 = dd.f32(6000, (n,), -9, 9)
    sm = dict(x=x0, eps=dd.normal_f16(6001, (n,), 1.0), D=np.zeros((n,), np.float16), noise=dd.f32(6002, (steps, n), -2, 2),
              coef=dd.f32(6003, (steps, 4), 0.1, 1.0), t_table=dd.f32(6004, (steps + 1,), 0, 999))
    for name, off in (("x", 4), ("eps", 2), ("D", 2), ("noise", 4), ("coef", 4)):
        b = _bufs(sm, {name: off})
        step, ts = torch.zeros(1, dtype=torch.int32, device=DEV), scal(-1.0)
        code = C._lib.mixdq_sampler_step(_p(b["x"]), _p(b["eps"]), _p(b["D"]), _p(b["noise"]), n, _p(b["coef"]),
                                         _p(b["t_table"]), steps, step.data_ptr(), ts.data_ptr(), 0.0, n, 1, n, _stream())
        assert _sync_status(code) == ERR_ALIGNMENT, f"sampler: {name} + {off}"
        assert b["D"].still_sentinel() and b["x"].untouched(), f"sampler: {name} + {off}"
        assert_bits(b["x"].value(), x0, "sampler state after a refused step")
        assert int(step.item()) == 0 and float(ts.item()) == -1.0


# =============================================================================================== module layer
@pytest.mark.parametrize("g", cg.GEOMETRIES + cg.REFUSED, ids=str)
def test_quantized_conv2d_module_geometry(C, oracle, g):
    """QuantizedConv2d.from_float(nn.Conv2d(16, 12, (R, S), stride, pad)): on the INT8 kernels == the oracle's
    quantize -> conv chain bit for bit, or (pad >= R or pad >= S) an FP fallback decided at construction; forward
    never raises."""
    from tests.test_conv_geometry_module_host import quantized_conv
    R, S, stride, pad = g
    qm, x = quantized_conv((R, S), (stride, stride), (pad, pad))
    assert qm.valid_for_acceleration == (pad < R and pad < S)
    qm = qm.half().to(DEV) if not qm.valid_for_acceleration else qm.to(DEV)
    with torch.no_grad():
        y = qm(x.half().to(DEV))
    if not qm.valid_for_acceleration:
        ref = torch.nn.functional.conv2d(x.double(), qm.weight.double().cpu(), qm.bias.double().cpu(), stride=stride, padding=pad)
        err = (y.double().cpu() - ref).abs()
        assert (err <= 2.0 ** -9 * ref.abs() + 2.0 ** -9 * ref.pow(2).mean().sqrt()).all()
        return
    variant = C.FLAGS & 1
    zp = float(qm.act_zero_points)
    xq = oracle.quantize(x.half().permute(0, 2, 3, 1).contiguous().numpy(), float(qm.act_scales_inv), zp, variant)
    wt = qm.weight_int.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    wsum = cg.wsum_of(wt)
    bias0 = None if pad else qm.bias0.cpu().numpy()
    want = oracle.qconv2d(xq, wt, qm.scale.cpu().numpy(), wsum if pad else None, zp, bias0, qm.bias.cpu().numpy(), stride,
                          pad, variant)
    assert_bits(y.permute(0, 2, 3, 1).contiguous(), want, f"module {g}")
