"""GPU tests of the FP16 layer kernels (mixdq_linear_f16, mixdq_conv2d_f16, mixdq_gemm_f16) on exact-result inputs
(tests/exact_inputs.py): integer-valued activations in [-4, 4] and weights in [-2, 2], bias a multiple of 1/8, K up to
5120, |acc| < 2^20 -- the FP32 accumulator and accumulator + bias are exact whatever the order of the sums, so the
output is fp16(acc + bias) [then fp16(f32(.) + f32(residual)): the residual is added after the rounding] and nothing
else.  Equality of BITS, no tolerance: a K tail piece staged twice, a dropped K-tile, a second rounding in the
epilogue (|acc + bias| reaches the range where FP16 spacing is 1/4 .. 1/2, ties included) are all red -- also when
every tile configuration shares them.
"""
import numpy as np
import pytest
import torch

from tests import exact_inputs as ei
from tests import tile_edges as te

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_bits(got, want, what):
    g, w = np.ascontiguousarray(got.cpu().numpy()).view(np.uint16), np.ascontiguousarray(want).view(np.uint16)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(int(x) for x in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ; first at {i}: got "
                             f"{got.cpu().numpy()[i]!r} want {np.asarray(want)[i]!r}")


F16L = te.all_f16()


@pytest.mark.parametrize("case", F16L, ids=[te.f16_id(c) for c in F16L])
def test_linear_f16_tile_edges_every_configuration_exact(C, case):
    M, N, K = case["M"], case["N"], case["K"]
    c = ei.linear(M, K, N, case["bias"], True)
    x, w, b, res = t(c["x"]), t(c["w"]), t(c["bias"]), t(c["residual"])
    plain = ei.f16_epilogue(c["x"].astype(np.float64) @ c["w"].astype(np.float64).T, c["bias"], None)
    for cfg in sorted(te.F16):
        assert_bits(C.linear_f16(x, w, b, _cfg=cfg), plain, f"linear_f16 cfg {cfg} m{M} n{N} k{K}")
        assert_bits(C.linear_f16(x, w, b, _residual=res, _cfg=cfg), c["expected"], f"linear_f16 + residual cfg {cfg}")


@pytest.mark.parametrize("M,K,N,bias", ei.LIN)
def test_linear_f16_layer_shapes_exact(C, M, K, N, bias):
    c = ei.linear(M, K, N, bias, False)
    x, w, b = t(c["x"]), t(c["w"]), t(c["bias"])
    assert_bits(C.linear_f16(x, w, b), c["expected"], f"linear_f16 m{M} n{N} k{K}")
    if M * N * K <= 1 << 28:
        for cfg in C.F16_CONFIGS:
            assert_bits(C.linear_f16(x, w, b, _cfg=cfg), c["expected"], f"linear_f16 cfg {cfg} m{M} n{N} k{K}")


@pytest.mark.parametrize("case", ei.CONV, ids=[f"c{c[1]}_k{c[4]}_{c[5]}x{c[5]}_s{c[6]}p{c[7]}" for c in ei.CONV])
def test_conv2d_f16_exact(C, case):
    N, Cin, H, W, K, ks, stride, pad, bias = case
    c = ei.conv2d(*case)
    x = t(c["x"])                                                   # NCHW memory
    xcl = x.contiguous(memory_format=torch.channels_last)
    w, b = t(c["w"]), t(c["bias"])
    what = f"conv2d_f16 c{Cin} k{K} {ks}x{ks} s{stride} p{pad}"
    out = C.conv2d_f16(xcl, w, b, stride, pad)
    assert_bits(out, c["expected"], what)
    assert_bits(C.conv2d_f16(x, w, b, stride, pad), c["expected"], what + " NCHW input")
    for cfg in C.F16_CONFIGS:
        assert_bits(C.conv2d_f16(xcl, w, b, stride, pad, _cfg=cfg), c["expected"], what + f" cfg {cfg}")
    full = ei.conv2d(*case, residual="full")
    r = t(full["residual"]).contiguous(memory_format=torch.channels_last)
    assert_bits(C.conv2d_f16(xcl, w, b, stride, pad, _residual=r), full["expected"], what + " + residual")
    per = ei.conv2d(*case, residual="per_image")
    assert_bits(C.conv2d_f16(xcl, w, b, stride, pad, _residual=t(per["residual"]), _residual_per_image=True),
                per["expected"], what + " + per-image residual")


@pytest.mark.parametrize("M,K,N", ei.GEMM)
def test_gemm_f16_exact(C, M, K, N):
    c = ei.gemm(M, K, N)
    assert_bits(C.qlinear_fp_reference(t(c["a"]), t(c["b"])), c["expected"], f"gemm_f16 m{M} k{K} n{N}")
