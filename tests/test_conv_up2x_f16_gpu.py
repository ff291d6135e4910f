"""GPU tests of mixdq_conv2d_f16 with MIXDQ_FLAG_UPSAMPLE2X (`_C.conv2d_f16(..., _upsample2x=True)`): diffusers'
`Upsample2D` -- a 3x3 conv on the nearest 2x upsampling of x -- without the upsampled tensor.  The gather of the MFMA
tiles reads pixel (y >> 1, x >> 1) of the small tensor: the same values land in the same tile, so the folded launch
must be BIT-equal to the conv on F.interpolate(x, 2, "nearest"), and both are held to the FP32-reference bound of
tests/test_f16_gpu.py:  |out - ref| <= 2^-10 * |ref| + 2^-10 * rms(ref).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_SHAPE = 9


def close(out, ref):
    ref = ref.to(out.device).float()
    tol = 2.0 ** -10 * ref.abs() + 2.0 ** -10 * ref.pow(2).mean().sqrt()
    err = (out.float() - ref).abs()
    bad = err > tol
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} outside tolerance; max err " \
                          f"{err.max().item():.3e} (tol there {tol.flatten()[err.argmax()].item():.3e})"


def rnd(shape, seed, std=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).half().to(DEV)


CASES = [  # N, h, w, C, K, residual
    (1, 5, 7, 32, 32, False), (2, 8, 8, 64, 128, False), (1, 3, 3, 8, 16, False), (1, 16, 16, 256, 256, True),
]


@pytest.mark.parametrize("case", CASES, ids=[f"n{c[0]}_{c[1]}x{c[2]}_c{c[3]}_k{c[4]}" + ("_res" if c[5] else "") for c in CASES])
def test_conv2d_f16_upsample2x_equals_the_conv_on_the_upsampled_tensor(C, case):
    N, h, w_, Cin, K, with_res = case
    x = rnd((N, Cin, h, w_), 40).contiguous(memory_format=torch.channels_last)
    w, b = rnd((K, Cin, 3, 3), 41, 0.05), rnd((K,), 42)
    res = rnd((N, K, 2 * h, 2 * w_), 43).contiguous(memory_format=torch.channels_last) if with_res else None
    up = F.interpolate(x, scale_factor=2, mode="nearest").contiguous(memory_format=torch.channels_last)
    assert tuple(up.shape) == (N, Cin, 2 * h, 2 * w_)
    want = C.conv2d_f16(up, w, b, 1, 1, _residual=res)
    got = C.conv2d_f16(x, w, b, 1, 1, _residual=res, _upsample2x=True)
    assert got.dtype == torch.float16 and tuple(got.shape) == (N, K, 2 * h, 2 * w_)
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    for cfg in C.F16_CONFIGS:                                # every tile of the family gathers the same way
        assert torch.equal(C.conv2d_f16(x, w, b, 1, 1, _residual=res, _cfg=cfg, _upsample2x=True), want), cfg
    ref = F.conv2d(F.interpolate(x.cpu().float(), scale_factor=2, mode="nearest"), w.cpu().float(), b.cpu().float(), 1, 1)
    if with_res:       # the residual is added after the FP16 rounding of the conv
        close(C.conv2d_f16(x, w, b, 1, 1, _upsample2x=True), ref)
        assert torch.equal(got, C.conv2d_f16(x, w, b, 1, 1, _upsample2x=True) + res)
    else:
        close(got, ref)


def _call(C, x, w, b, out, H, W, R, S, stride, pad):
    N, Cin, K = x.shape[0], x.shape[1], w.shape[0]
    return C._lib.mixdq_conv2d_f16(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), N, H, W, Cin, K, R, S,
                                   stride, pad, None, 1, C.FLAG_UPSAMPLE2X, None)


def test_conv2d_f16_upsample2x_refuses_other_geometry_and_writes_nothing(C):
    """3x3 / stride 1 / pad 1, even H and W, on the MFMA tiles: a 1x1 kernel, stride 2, pad 0, an odd size and a
    channel count the tiles do not take answer MIXDQ_ERR_SHAPE with the output buffer untouched."""
    x = rnd((1, 16, 4, 4), 50).contiguous(memory_format=torch.channels_last)
    b = rnd((16,), 52)
    w3 = rnd((16, 16, 3, 3), 51, 0.05).contiguous(memory_format=torch.channels_last)
    w1 = rnd((16, 16, 1, 1), 53, 0.05).contiguous(memory_format=torch.channels_last)
    sentinel = 0x5a5a
    out = torch.full((1, 8, 8, 16), sentinel, dtype=torch.int16, device=DEV)
    assert _call(C, x, w3, b, out, 8, 8, 3, 3, 1, 1) == 0                    # the accepted geometry
    torch.cuda.synchronize()
    assert not bool((out == sentinel).all())
    for name, args in (("1x1", (w1, 8, 8, 1, 1, 1, 0)), ("stride 2", (w3, 8, 8, 3, 3, 2, 1)),
                       ("pad 0", (w3, 8, 8, 3, 3, 1, 0)), ("odd H", (w3, 7, 8, 3, 3, 1, 1))):
        out.fill_(sentinel)
        wt, *geo = args
        assert _call(C, x, wt, b, out, *geo) == ERR_SHAPE, name
        torch.cuda.synchronize()
        assert bool((out == sentinel).all()), name
    x4 = rnd((1, 4, 4, 4), 54).contiguous(memory_format=torch.channels_last)   # C = 4: the one-output-per-thread kernel
    w4 = rnd((16, 4, 3, 3), 55, 0.05).contiguous(memory_format=torch.channels_last)
    out.fill_(sentinel)
    assert _call(C, x4, w4, b, out, 8, 8, 3, 3, 1, 1) == ERR_SHAPE
    with pytest.raises(RuntimeError, match="shape outside"):
        C.conv2d_f16(x, w1, b, 1, 0, _upsample2x=True)
    with pytest.raises(RuntimeError, match="shape outside"):
        C.conv2d_f16(x, w3, b, 2, 1, _upsample2x=True)
