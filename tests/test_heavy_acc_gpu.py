"""Every INT8 launch on accumulators FP32 cannot hold (operands: tests/heavy_acc.py; tests/test_heavy_acc_host.py checks
them and the references on the CPU).  The first statement of every INT8 epilogue is f32(acc), round to nearest even --
csrc/common.h epilogue_one (the generic kernels), csrc/igemm_kernel.h (the GEMM + GEGLU epilogue; the tile epilogue of
the whole family, and with it the f16in, LN, grouped, row-map and to_q + attention launches), csrc/igemm_pp.h (the
persistent kernel's two epilogues), csrc/iconv.hip (the halo conv) -- and no other suite hands a kernel an accumulator
that conversion has to round.

Every comparison is bit equality, with an integer computed without floats (scale 1, no bias: RNE(acc) - base, an
FP16 number) or with the oracle's bits (the second operand set: per-column scales down to the FP16 subnormals and up
past 65504, an FP16 bias, integer residuals).  Outputs go into NaN-filled (INT8: -128-filled) buffers wherever the
binding takes one.  Both epilogue variants."""
import functools

import numpy as np
import pytest
import torch

from tests import heavy_acc as ha
from tests import tile_edges as te

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True, params=["A", "B"], ids=["fma", "mul_add"])
def epilogue_variant(request, monkeypatch):
    """Both roundings of the epilogue's multiply-add (tests/test_ops_gpu.py)."""
    import mixdq_amd._C as C_
    monkeypatch.setattr(C_, "FLAGS", 1 if request.param == "B" else 0)
    return request.param


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scal(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def nan_buffer(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float16, device=DEV)


def bits_equal(got, want, what):
    """`want`: uint16 FP16 bit patterns, an FP16 array, or int8."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    g = got.view(np.uint16) if got.dtype == np.float16 else got
    w = want.view(np.uint16) if want.dtype == np.float16 else want
    assert g.shape == w.shape, f"{what}: shape {g.shape} vs {w.shape}"
    bad = np.nonzero(g.reshape(-1) != w.reshape(-1))[0]
    assert bad.size == 0, (f"{what}: {bad.size}/{g.size} elements differ; first at flat index {bad[0]}: "
                           f"got {g.reshape(-1)[bad[0]]:#x} want {w.reshape(-1)[bad[0]]:#x}")


def gemm(C, c, w=None, scale=None, bias=None, **kw):
    """qlinear_w8_a8_ohalf (mixdq_qlinear_w8a8_rows) on a heavy_acc.Linear, into a NaN-filled buffer."""
    out = kw.pop("_out", None)
    if out is None:
        out = nan_buffer(c.M, c.N)
    sc, b0 = t(c.scale if scale is None else scale), t(c.bias0)
    C.qlinear_w8_a8_ohalf(t(c.a), t(c.w) if w is None else w, sc, scal(1), scal(ha.ZP), b0, sc, b0,
                          None if bias is None else t(bias), _out=out, **kw)
    return out


@functools.lru_cache(maxsize=None)
def fp16_end_linear(case, variant):
    """(scale, bias, residual, the oracle's output, the oracle's output + residual) of the second operand set."""
    from oracle import oracle as O
    c = ha.linear(*case)
    scale, bias, residual, _ = ha.fp16_end(c)
    want = O.qlinear(c.a, c.w, c.bias0, scale, bias, variant)
    return scale, bias, residual, want, O.add_f16(want, residual)


def residual_of(c):
    """Integer residuals and the integer expectation of (RNE(acc) - base) + residual."""
    r = np.random.default_rng(c.M + c.N).integers(-64, 65, c.want_int.shape)
    return ha.f16_bits(r).view(np.float16), ha.f16_bits(c.want_int + r)


# ------------------------------------------------------------------------------------- GEMM: every tile
TILE_SHAPES = [(cfg, shape) for cfg in ha.int8_tiles() for shape in ha.gemm_shapes(cfg)]


@pytest.mark.parametrize("cfg,shape", TILE_SHAPES, ids=[f"cfg{c}_m{s[0]}_n{s[1]}_k{s[2]}" for c, s in TILE_SHAPES])
def test_gemm_every_tile(C, cfg, shape):
    """Forced tile, plain and with the residual epilogue; the automatic choice at the same shape; the second set."""
    c = ha.linear(*shape)
    bits_equal(gemm(C, c, _cfg=cfg), c.want, f"cfg {cfg}")
    bits_equal(gemm(C, c), c.want, f"automatic choice at cfg {cfg}'s shape")
    r, want_r = residual_of(c)
    bits_equal(gemm(C, c, _cfg=cfg, _residual=t(r)), want_r, f"cfg {cfg}, residual epilogue")
    scale, bias, res2, want2, want2_r = fp16_end_linear(shape + (-128, False), C.FLAGS & 1)
    bits_equal(gemm(C, c, scale=scale, bias=bias, _cfg=cfg), want2, f"cfg {cfg}, FP16 end")
    bits_equal(gemm(C, c, scale=scale, bias=bias, _cfg=cfg, _residual=t(res2)), want2_r, f"cfg {cfg}, FP16 end + residual")


def test_generic_linear_kernel(C):
    """K % 16 != 0: the one-output-per-thread kernel (csrc/common.h epilogue_one)."""
    M, N, K = ha.GENERIC_LINEAR
    assert C.igemm_select_id(M, N, K) == 0
    c = ha.linear(M, N, K)
    bits_equal(gemm(C, c), c.want, "generic")
    scale, bias, res2, want2, want2_r = fp16_end_linear((M, N, K, -128, False), C.FLAGS & 1)
    bits_equal(gemm(C, c, scale=scale, bias=bias), want2, "generic, FP16 end")
    bits_equal(gemm(C, c, scale=scale, bias=bias, _residual=t(res2)), want2_r, "generic, FP16 end + residual")


def test_row_map(C):
    """mixdq_qlinear_w8a8_rows with a row map: g groups of rows, each behind one row the launch must not touch."""
    cfg = min(te.IGEMM)
    c = ha.linear(*ha.gemm_shape(cfg))
    g = next(d for d in (13, 7, 5, 3, 2, 1) if c.M % d == 0)
    rows = c.M // g
    out = nan_buffer(g, rows + 1, c.N)
    gemm(C, c, _out=out, _row_map=(rows, rows + 1, 1))
    bits_equal(out[:, 1:].reshape(c.M, c.N), c.want, "row map")
    assert bool(torch.isnan(out[:, 0]).all()), "a row outside the map was written"


@pytest.mark.parametrize("cfg", sorted(te.GROUPED))
def test_grouped_launch(C, cfg):
    """One grouped launch: every class in every member (N = BN - 4, BN + 4, 2 BN + 4: three sets of weights on the same
    activations)."""
    cases = [ha.linear(*shape) for shape in ha.grouped_shapes(cfg)]
    outs = [nan_buffer(c.M, c.N) for c in cases]
    assert all(np.array_equal(c.a, cases[0].a) for c in cases)
    table = C.GemmGroupTable([(t(c.w), t(c.bias0), t(c.scale), None, o) for c, o in zip(cases, outs)])
    C.qlinear_grouped(t(cases[0].a), table, _cfg=cfg)
    for i, (c, o) in enumerate(zip(cases, outs)):
        bits_equal(o, c.want, f"member {i} (N = {c.N}), cfg {cfg}")


@pytest.mark.parametrize("cfg", sorted(te.AQ))
def test_f16in(C, cfg):
    """The quantizing family: FP16 values 0, 1, 3, 5 with scale_inv 1 and zp -128 quantize to the same operand."""
    bm, bn, bk, st = te.tile(cfg, te.AQ)
    c = ha.linear(bm + 1, bn + 4, ha.K_INT8)
    x = (c.a.astype(np.int16) + 128).astype(np.float16)
    out = nan_buffer(c.M, c.N)
    C.qlinear_f16in(t(x), scal(1), scal(ha.ZP), t(c.w), t(c.scale), t(c.bias0), None, _out=out, _cfg=cfg)
    bits_equal(out, c.want, f"f16in cfg {cfg}")


@pytest.mark.parametrize("cfg", ha.LN_TILES)
def test_ln_launch(C, oracle, cfg):
    """GEMM + LayerNorm + quantize in one launch: its FP16 rows are the integer expectation, its quantized outputs the
    oracle's layernorm_quantize of those rows."""
    c = ha.linear(te.tile(cfg)[0] + 1, ha.LN_N, ha.K_INT8)
    rng = np.random.default_rng(cfg)
    gamma = (1 + 0.3 * rng.standard_normal(c.N)).astype(np.float16)
    beta = (0.2 * rng.standard_normal(c.N)).astype(np.float16)
    qp = [(float(np.float32(1) / np.float32(0.02)), -7.0), (float(np.float32(1) / np.float32(0.03)), 4.0)]
    ws = C.qlinear_ln_workspace(c.M, c.N, DEV)
    y, outs, _ = C.qlinear_ln(t(c.a), t(c.w), t(c.scale), t(c.bias0), None, None, t(gamma), t(beta), 1e-5,
                              [(scal(a), scal(b)) for a, b in qp], ws, _cfg=cfg)
    bits_equal(y, c.want, f"LN cfg {cfg}: FP16 rows")
    q_ref, _ = oracle.layernorm_quantize(c.want.view(np.float16), gamma, beta, 1e-5, qp, C.FLAGS & 1)
    for i, (got, want) in enumerate(zip(outs, q_ref)):
        bits_equal(got, want, f"LN cfg {cfg}: quantizer {i}")
    assert C.qlinear_ln_status(ws) == 0


PACKED = [(bits, cfg) for bits in (4, 2) for cfg in ha.packed_tiles(bits) + [0]]


@pytest.mark.parametrize("bits,cfg", PACKED, ids=[f"w{b}_cfg{c}" for b, c in PACKED])
def test_packed_weights(C, bits, cfg):
    """W4 / W2: the MFMA runs on 16 q / 64 q, the epilogue on 16 bias0 and scale / 16 (64): exact, says a comment."""
    from mixdq_amd.nn.utils import pack_w2, pack_w4
    qmin, K = (-8, ha.K_W4) if bits == 4 else (-2, ha.K_W2)
    bn = te.tile(cfg or ha.packed_tiles(bits)[0])[1]
    c = ha.linear(5, bn + 4, K, qmin)
    packed = (pack_w4 if bits == 4 else pack_w2)(torch.from_numpy(c.w)).to(DEV)
    kw = dict(_w4=True) if bits == 4 else dict(_w2=True)
    bits_equal(gemm(C, c, w=packed, _cfg=cfg, **kw), c.want, f"W{bits} cfg {cfg}")
    scale, bias, res2, want2, want2_r = fp16_end_linear((5, bn + 4, K, qmin, False), C.FLAGS & 1)
    bits_equal(gemm(C, c, w=packed, scale=scale, bias=bias, _cfg=cfg, _residual=t(res2), **kw), want2_r,
               f"W{bits} cfg {cfg}, FP16 end + residual")


# --------------------------------------------------------------------------------------- GEMM + GEGLU
def geglu(C, c, cfg, **kw):
    D = c.N // 2
    perm = C.geglu_row_order(D, DEV)
    w = kw.pop("w", None)
    w = t(c.w)[perm].contiguous() if w is None else w
    out = torch.full((c.M, D), -128, dtype=torch.int8, device=DEV)           # |expectation| <= 127: never -128
    C.qlinear_geglu(t(c.a), w, t(c.scale)[perm].contiguous(), t(c.bias0)[perm].contiguous(),
                    t(c.bias)[perm].contiguous(), scal(1.0 / 16), scal(0), _cfg=cfg, _out=out, **kw)
    return out


@pytest.mark.parametrize("cfg", [c for c in ha.int8_tiles() if te.geglu_admissible(c)])
def test_geglu_every_admissible_tile(C, cfg):
    """Gate columns: zero weights and bias 16, gelu(16) == 16 (checked on the CPU); quantizer 1/16, zp 0: the INT8
    output is the integer expectation itself."""
    c = ha.linear(*ha.geglu_shape(cfg), -128, True)
    bits_equal(geglu(C, c, cfg), c.want_q, f"GEGLU cfg {cfg}")


def test_geglu_w4(C):
    from mixdq_amd.nn.utils import pack_w4
    c = ha.linear(5, 96, ha.K_W4, -8, True)
    perm = C.geglu_row_order(c.N // 2, "cpu")
    packed = pack_w4(torch.from_numpy(c.w)[perm].contiguous()).to(DEV)
    bits_equal(geglu(C, c, 0, w=packed, _w4=True), c.want_q, "GEGLU W4")


# ----------------------------------------------------------------------------------------------- conv
def conv_args(c, scale=None, bias=None, w=None, x=None):
    K = c.K
    sc = t(c.scale if scale is None else scale)
    return (t(c.x if x is None else x).permute(0, 3, 1, 2), t(c.w).permute(0, 3, 1, 2) if w is None else w, sc, scal(1),
            scal(ha.ZP), sc, t(c.wsum.reshape(K, 1, 3, 3)), None, None if bias is None else t(bias), 1, 1)


def nhwc(out):
    return out.permute(0, 2, 3, 1).contiguous().cpu().numpy()


@functools.lru_cache(maxsize=None)
def fp16_end_conv(case, variant):
    from oracle import oracle as O
    c = ha.conv(*case)
    scale, bias, _, _ = ha.fp16_end(c)
    rng = np.random.default_rng(c.K)
    full = rng.integers(-64, 65, c.acc.shape).astype(np.float16)
    image = rng.integers(-64, 65, (c.n, c.K)).astype(np.float16)
    want = O.qconv2d(c.x, c.w, scale, c.wsum, float(ha.ZP), None, bias, 1, 1, variant)
    assert not np.isnan(want).any()
    return scale, bias, full, image, want, O.add_f16(want, full), O.add_f16(want, np.broadcast_to(image[:, None, None, :],
                                                                                                 want.shape))


def conv_fp16_end(C, c, case, cfg, what, **kw):
    scale, bias, full, image, want, want_full, want_image = fp16_end_conv(case, C.FLAGS & 1)
    args = conv_args(c, scale, bias, **kw)
    bits_equal(nhwc(C.qconv2d_w8_a8_ohalf(*args, _cfg=cfg)), want, f"{what}, FP16 end")
    r = t(full).permute(0, 3, 1, 2)
    bits_equal(nhwc(C.qconv2d_w8_a8_ohalf(*args, _cfg=cfg, _residual=r)), want_full, f"{what}, FP16 end + residual")
    bits_equal(nhwc(C.qconv2d_w8_a8_ohalf(*args, _cfg=cfg, _residual=t(image), _residual_per_image=True)), want_image,
               f"{what}, FP16 end + per-image residual")


@pytest.mark.parametrize("cfg", ha.int8_tiles())
def test_conv_every_implicit_gemm_tile(C, cfg):
    case = ha.CONV_SHAPE + (ha.CONV_C, ha.conv_k(te.tile(cfg)[1]), -128)
    c = ha.conv(*case)
    bits_equal(nhwc(C.qconv2d_w8_a8_ohalf(*conv_args(c), _cfg=cfg)), c.want, f"conv cfg {cfg}")
    conv_fp16_end(C, c, case, cfg, f"conv cfg {cfg}")


@pytest.mark.parametrize("tile", sorted(ha.HALO))
def test_conv_halo_tiles(C, tile):
    """The halo kernel's tiles, W8 and packed W4, forced; the automatic choice and the border-table entry point at the
    same shape."""
    from mixdq_amd.nn.utils import pack_w4
    k = ha.conv_k(ha.HALO[tile][2])
    case = ha.CONV_SHAPE + (ha.CONV_C, k, -128)
    c = ha.conv(*case)
    assert C.conv_halo_select(c.n, c.H, c.W, c.C, k, 3, 3, 1, 1) in ha.HALO
    bits_equal(nhwc(C.qconv2d_w8_a8_ohalf(*conv_args(c), _cfg=tile)), c.want, f"halo tile {tile}")
    bits_equal(nhwc(C.qconv2d_w8_a8_ohalf(*conv_args(c))), c.want, f"automatic choice at halo tile {tile}'s shape")
    table = C.conv_border_table(t(c.wsum.reshape(k, 1, 3, 3)))
    bits_equal(nhwc(C.qconv2d_w8_a8_ohalf(*conv_args(c), _table=table)), c.want, "mixdq_qconv2d_w8a8_table")
    conv_fp16_end(C, c, case, tile, f"halo tile {tile}")
    c4 = ha.conv(*ha.CONV_W4_SHAPE, ha.CONV_W4_C, k, -8)
    assert C.conv_halo_select(c4.n, c4.H, c4.W, c4.C, k, 3, 3, 1, 1, w4=True) in ha.HALO
    w4 = pack_w4(torch.from_numpy(c4.w)).to(DEV).permute(0, 3, 1, 2)
    bits_equal(nhwc(C.qconv2d_w8_a8_ohalf(*conv_args(c4, w=w4), _cfg=tile, _w4=True)), c4.want, f"W4 halo tile {tile}")


def test_conv_upsample_fold(C):
    """conv(nearest-2x-upsample(x)) read from the small tensor, on every halo tile."""
    for tile in sorted(ha.HALO):
        c = ha.conv(*ha.CONV_SHAPE, ha.CONV_C, ha.conv_k(ha.HALO[tile][2]), -128, True)
        assert C.conv_upsample2x_supported((c.n, c.C, c.H // 2, c.W // 2), (c.K, c.C, 3, 3), 1, 1)
        got = C.qconv2d_w8_a8_ohalf(*conv_args(c, x=c.x_small), _cfg=tile, _upsample2x=True)
        bits_equal(nhwc(got), c.want, f"upsample fold, tile {tile}")


def test_conv_w4_implicit_gemm(C):
    from mixdq_amd.nn.utils import pack_w4
    cfg = min(te.IGEMM)
    c4 = ha.conv(*ha.CONV_W4_SHAPE, ha.CONV_W4_C, ha.conv_k(ha.HALO[min(ha.HALO)][2]), -8)
    w4 = pack_w4(torch.from_numpy(c4.w)).to(DEV).permute(0, 3, 1, 2)
    bits_equal(nhwc(C.qconv2d_w8_a8_ohalf(*conv_args(c4, w=w4), _cfg=cfg, _w4=True)), c4.want, f"W4 conv cfg {cfg}")


def test_generic_conv_kernel(C):
    """C % 16 != 0 with R S C >= 1032: the one-output-per-thread conv (csrc/common.h epilogue_one)."""
    n, H, W, Cin, K = ha.GENERIC_CONV
    assert Cin % 16 != 0 and 9 * Cin >= 1032 and C.igemm_select_id(n * H * W, K, Cin, 9 * Cin) == 0
    c = ha.conv(n, H, W, Cin, K)
    bits_equal(nhwc(C.qconv2d_w8_a8_ohalf(*conv_args(c))), c.want, "generic conv")
