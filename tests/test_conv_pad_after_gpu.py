"""GPU tests of mixdq_conv2d_f16 with MIXDQ_FLAG_PAD_AFTER (`_C.conv2d_f16(..., _pad_after=True)`): the zero padding
lies below and right of the image only -- diffusers' `Downsample2D` in a VAE, a 3x3 / stride 2 conv over
F.pad(x, (0, 1, 0, 1)) -- without the padded tensor.  M, N and K are those of the conv on the padded tensor and the same
values land in the same tile slots (a tap outside the image is the same zero either way), so the flagged launch must
be BIT-equal to `conv2d_f16(F.pad(x, (0, 1, 0, 1)), w, b, stride, 0)`: on the MFMA tiles, on every forced tile, on the
one-output-per-thread kernel, with and without a residual."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_UNSUPPORTED, ERR_SHAPE = 3, 9


def rnd(shape, seed, std=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).half().to(DEV)


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _operands(N, H, W, Cin, K, stride, with_res, seed=60):
    x = cl(rnd((N, Cin, H, W), seed))
    w, b = rnd((K, Cin, 3, 3), seed + 1, 0.05), rnd((K,), seed + 2)
    padded = cl(F.pad(x, (0, 1, 0, 1)))
    P, Q = (H + 1 - 3) // stride + 1, (W + 1 - 3) // stride + 1
    res = cl(rnd((N, K, P, Q), seed + 3)) if with_res else None
    return x, w, b, padded, res, (P, Q)


CASES = [(1, 8, 8, 32, 32), (2, 7, 9, 32, 64), (2, 16, 12, 8, 32)]       # N, H, W, C, K: the MFMA tiles


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("stride", [2, 1])
@pytest.mark.parametrize("case", CASES, ids=[f"n{c[0]}_{c[1]}x{c[2]}_c{c[3]}_k{c[4]}" for c in CASES])
def test_pad_after_equals_the_conv_on_the_padded_tensor(C, case, stride, with_res):
    N, H, W, Cin, K = case
    x, w, b, padded, res, (P, Q) = _operands(N, H, W, Cin, K, stride, with_res)
    want = C.conv2d_f16(padded, w, b, stride, 0, _residual=res)
    got = C.conv2d_f16(x, w, b, stride, 1, _residual=res, _pad_after=True)
    assert got.dtype == torch.float16 and tuple(got.shape) == (N, K, P, Q) == tuple(want.shape)
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert same(got, want)
    # it is not the symmetric conv (whose window starts one pixel up and left), and it is the conv: FP32 on the CPU
    sym = C.conv2d_f16(x, w, b, stride, 1)
    assert tuple(sym.shape) != tuple(got.shape) or not same(sym, got)
    ref = F.conv2d(F.pad(x.cpu().float(), (0, 1, 0, 1)), w.cpu().float(), b.cpu().float(), stride, 0)
    plain = got if res is None else C.conv2d_f16(x, w, b, stride, 1, _pad_after=True)
    tol = 2.0 ** -10 * ref.abs() + 2.0 ** -10 * ref.pow(2).mean().sqrt()          # tests/test_f16_gpu.py's bound
    assert bool(((plain.cpu().float() - ref).abs() <= tol).all())
    if res is not None:        # the residual is added after the FP16 rounding of the conv
        assert same(got, plain + res)


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
def test_pad_after_on_every_forced_tile(C, with_res):
    N, H, W, Cin, K = 2, 7, 9, 32, 64
    for stride in (2, 1):
        x, w, b, padded, res, _ = _operands(N, H, W, Cin, K, stride, with_res, seed=70)
        want = C.conv2d_f16(padded, w, b, stride, 0, _residual=res)
        for cfg in C.F16_CONFIGS:
            assert same(C.conv2d_f16(padded, w, b, stride, 0, _residual=res, _cfg=cfg), want), cfg
            assert same(C.conv2d_f16(x, w, b, stride, 1, _residual=res, _cfg=cfg, _pad_after=True), want), (cfg, stride)


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("stride", [2, 1])
def test_pad_after_on_the_one_output_per_thread_kernel(C, stride, with_res):
    """C = 4 (2C % 16 != 0) and K = 6 (K % 4 != 0): neither takes the tiles."""
    for Cin, K in ((4, 32), (32, 6), (4, 6)):
        x, w, b, padded, res, (P, Q) = _operands(2, 7, 9, Cin, K, stride, with_res, seed=80)
        want = C.conv2d_f16(padded, w, b, stride, 0, _residual=res)
        got = C.conv2d_f16(x, w, b, stride, 1, _residual=res, _pad_after=True)
        assert tuple(got.shape) == (2, K, P, Q) and same(got, want), (Cin, K)


def test_pad_after_other_windows(C):
    """Beyond 3x3 / pad 1: a 5x5 window with two rows of zeros, and pad 0, where the flag changes nothing."""
    x = cl(rnd((1, 16, 9, 10), 90))
    w5, b = rnd((32, 16, 5, 5), 91, 0.05), rnd((32,), 92)
    assert same(C.conv2d_f16(x, w5, b, 2, 2, _pad_after=True), C.conv2d_f16(cl(F.pad(x, (0, 2, 0, 2))), w5, b, 2, 0))
    w3 = rnd((32, 16, 3, 3), 93, 0.05)
    assert same(C.conv2d_f16(x, w3, b, 2, 0, _pad_after=True), C.conv2d_f16(x, w3, b, 2, 0))


def _conv_f16(C, x, w, b, out, H, W, R, S, stride, pad, flags):
    N, Cin, K = x.shape[0], x.shape[1], w.shape[0]
    return C._lib.mixdq_conv2d_f16(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), N, H, W, Cin, K, R, S,
                                   stride, pad, None, 1, flags, None)


def test_pad_after_refusals_write_nothing(C):
    sentinel = 0x5a5a
    x = cl(rnd((1, 16, 4, 4), 50))
    b = rnd((16,), 52)
    w3, w1 = cl(rnd((16, 16, 3, 3), 51, 0.05)), cl(rnd((16, 16, 1, 1), 53, 0.05))
    out = torch.full((1, 8, 8, 16), sentinel, dtype=torch.int16, device=DEV)
    assert _conv_f16(C, x, w3, b, out, 4, 4, 3, 3, 2, 1, C.FLAG_PAD_AFTER) == 0            # the accepted form: 2 x 2 pixels
    torch.cuda.synchronize()
    flat = out.view(-1)
    assert not bool((flat[:2 * 2 * 16] == sentinel).all()) and bool((flat[2 * 2 * 16:] == sentinel).all())
    for name, args in (("with the upsample fold", (w3, 8, 8, 3, 3, 1, 1, C.FLAG_PAD_AFTER | C.FLAG_UPSAMPLE2X)),
                       ("pad >= R", (w1, 4, 4, 1, 1, 1, 1, C.FLAG_PAD_AFTER)),
                       ("pad >= S", (w3, 4, 4, 3, 3, 1, 3, C.FLAG_PAD_AFTER))):
        out.fill_(sentinel)
        wt, *geo = args
        assert _conv_f16(C, x, wt, b, out, *geo) == ERR_SHAPE, name
        torch.cuda.synchronize()
        assert bool((out == sentinel).all()), name
    with pytest.raises(RuntimeError, match="shape outside"):
        C.conv2d_f16(x, w3, b, 1, 1, _upsample2x=True, _pad_after=True)

    # the INT8 convs refuse the flag: their zero-point border table is built for symmetric padding
    xi = torch.zeros((1, 4, 4, 16), dtype=torch.int8, device=DEV)
    wi = torch.zeros((16, 3, 3, 16), dtype=torch.int8, device=DEV)
    scale = torch.ones(16, dtype=torch.float32, device=DEV)
    wsum = torch.zeros(16 * 9, dtype=torch.float32, device=DEV)
    zp = torch.zeros(1, dtype=torch.float32, device=DEV)
    ws = torch.full((81 * 16,), 7.0, dtype=torch.float32, device=DEV)             # R*R*S*S*K floats: the border table
    out.fill_(sentinel)
    code = C._lib.mixdq_qconv2d_w8a8(xi.data_ptr(), wi.data_ptr(), scale.data_ptr(), wsum.data_ptr(), zp.data_ptr(),
                                     None, None, out.data_ptr(), ws.data_ptr(), 1, 4, 4, 16, 16, 3, 3, 2, 1, 1,
                                     C.FLAG_PAD_AFTER, None)
    assert code == ERR_UNSUPPORTED
    code = C._lib.mixdq_qconv2d_w8a8_table(xi.data_ptr(), wi.data_ptr(), scale.data_ptr(), ws.data_ptr(), zp.data_ptr(),
                                           None, None, out.data_ptr(), 1, 4, 4, 16, 16, 3, 3, 2, 1, None, 1,
                                           C.FLAG_PAD_AFTER, None)
    assert code == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()) and bool((ws == 7.0).all())
