"""GPU tests of the FP16 attention core at SD 1.5's head widths (40, 80, 160: attn_hd_kernel).

The same criteria as tests/test_attention_gpu.py: |got - ref| <= 2e-3 + 4e-3 |ref| against the float64 oracle, no
further from it than PyTorch's FP16 SDPA (max and RMS), the INT8 output equal to quantize() of the kernel's own FP16
output; every form of a width (128- and 64-query workgroups) and every batch row bit-identical; other widths refused.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import detdata as dd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL, RTOL = 2e-3, 4e-3
WIDTHS = (40, 80, 160)
S_INV, ZP = float(np.float32(1) / np.float32(0.0173)), 7.0


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scal(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def make(seed, B, tq, tkv, C, fused):
    """Host q/k/v and their device views: `fused` = one [B, T, 3C] q|k|v buffer (self-attention) or a [B, Tkv, 2C]
    k|v buffer: column slices with a row stride, as in the UNet."""
    if fused and tq == tkv:
        qkv = dd.normal_f16(seed, (B, tq, 3 * C), 1.2)
        d = t(qkv)
        return (qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]), (d[..., :C], d[..., C:2 * C], d[..., 2 * C:])
    q = dd.normal_f16(seed, (B, tq, C), 1.2)
    kv = dd.normal_f16(seed + 1, (B, tkv, 2 * C), 1.2)
    qd, kvd = t(q), t(kv)
    return (q, kv[..., :C], kv[..., C:]), (qd, kvd[..., :C], kvd[..., C:])


def sdpa(q, k, v, heads, D):
    B, tq, C = q.shape
    return F.scaled_dot_product_attention(*(x.unflatten(-1, (heads, D)).transpose(1, 2) for x in (q, k, v))
                                          ).transpose(1, 2).reshape(B, tq, C)


SHAPES = [  # B, Tq, Tkv, heads, fused layout
    (1, 128, 64, 2, False),
    (2, 100, 77, 3, False),        # ragged queries, 77 keys (cross-attention)
    (2, 96, 130, 2, False),        # ragged keys past two tiles
    (3, 33, 1, 2, False),          # a single key: out == v
    (1, 1, 300, 2, False),         # a single query
    (2, 256, 256, 3, True),        # fused q|k|v
    (1, 64, 640, 1, True),         # 10 key tiles: the two-stage ring wraps
    (2, 200, 77, 8, False),        # SD 1.5's 8 heads
]
CASES = [(D, cfg) + s for D in WIDTHS for cfg in (0, 2, 4) for s in SHAPES]


def _id(c):
    return f"d{c[0]}_w{c[1]}_b{c[2]}_q{c[3]}_k{c[4]}_h{c[5]}_{'f' if c[6] else 's'}"


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_attention_hd_vs_oracle(C, oracle, case):
    D, cfg, B, tq, tkv, heads, fused = case
    Cc = heads * D
    (q, k, v), (qd, kd, vd) = make(31 + D, B, tq, tkv, Cc, fused)
    _, ref64 = oracle.attention_f16(q, k, v, heads)
    got = C.attention_f16(qd, kd, vd, heads, _cfg=cfg)
    assert got.shape == (B, tq, Cc) and got.dtype == torch.float16 and got.is_contiguous()
    g = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all()
    err = np.abs(g - ref64)
    assert (err <= ATOL + RTOL * np.abs(ref64)).all(), f"max err {err.max():.3e}"
    err_sd = np.abs(sdpa(qd, kd, vd, heads, D).cpu().numpy().astype(np.float64) - ref64)
    assert err.max() <= 1.5 * err_sd.max() + 1e-3
    assert np.sqrt((err ** 2).mean()) <= 1.5 * np.sqrt((err_sd ** 2).mean()) + 1e-5
    if tkv == 1:
        assert torch.equal(got, vd.expand(B, tq, Cc).contiguous())


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("shape", [(2, 100, 77, 3, False), (2, 256, 256, 2, True), (1, 64, 640, 1, True)],
                         ids=["cross77", "self256", "k640"])
def test_attention_hd_int8_output_is_quantize_of_fp16_output(C, oracle, D, shape):
    B, tq, tkv, heads, fused = shape
    Cc = heads * D
    _, (qd, kd, vd) = make(41 + D, B, tq, tkv, Cc, fused)
    o16 = C.attention_f16(qd, kd, vd, heads)
    for unfused in (0, 1):
        flags = C.FLAGS
        try:
            C.FLAGS = (flags & ~1) | unfused
            o8 = C.attention_f16(qd, kd, vd, heads, scal(S_INV), scal(ZP))
            o4 = C.attention_f16(qd, kd, vd, heads, scal(S_INV), scal(ZP), _abits=4)
            q8 = C.quantize_per_tensor_to_int8(o16, scal(S_INV), scal(ZP))
        finally:
            C.FLAGS = flags
        assert o8.dtype == torch.int8 and o8.shape == o16.shape
        want = oracle.quantize(o16.cpu().numpy(), S_INV, ZP, unfused)
        assert np.array_equal(o8.cpu().numpy(), want) and torch.equal(o8, q8)
        assert (want != want.flat[0]).any()
        assert torch.equal(o4, q8.clamp(max=-113))
        assert int(o4.min()) >= -128 and int(o4.max()) <= -113
        for cfg in (2, 4):                       # every form, INT8 output too
            assert torch.equal(C.attention_f16(qd, kd, vd, heads, scal(S_INV), scal(ZP), _cfg=cfg), o8)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("tkv", [77, 300])
def test_attention_hd_forms_agree_and_batch_rows_equal_single_runs(C, D, tkv):
    B, tq, heads = 3, 320, 2
    Cc = heads * D
    _, (qd, kd, vd) = make(77 + D, B, tq, tkv, Cc, False)
    auto = C.attention_f16(qd, kd, vd, heads)
    assert torch.equal(auto, C.attention_f16(qd, kd, vd, heads, _cfg=4))
    assert torch.equal(auto, C.attention_f16(qd, kd, vd, heads, _cfg=2))
    assert torch.equal(auto, C.attention_f16(qd, kd, vd, heads, softmax_scale=D ** -0.5))
    for b in range(B):
        assert torch.equal(C.attention_f16(qd[b:b + 1], kd[b:b + 1], vd[b:b + 1], heads), auto[b:b + 1])
    other = C.attention_f16(qd, kd, vd, heads, softmax_scale=0.1)
    assert not torch.equal(other, auto)          # the scale argument is honoured


FULL = [  # SD 1.5 at 512 px, 8 heads: (Tq, Tkv, C)
    (4096, 4096, 320), (1024, 1024, 640), (256, 256, 1280), (4096, 77, 320), (1024, 77, 640), (256, 77, 1280),
]


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("case", FULL, ids=[f"q{c[0]}_k{c[1]}_c{c[2]}" for c in FULL])
def test_attention_hd_full_size_vs_torch_fp32(C, case, B):
    tq, tkv, Cc = case
    heads = 8
    D = Cc // heads
    g = torch.Generator(device="cpu").manual_seed(5)
    if tq == tkv:
        qkv = (torch.randn(B, tq, 3 * Cc, generator=g) * 1.3).half().to(DEV)
        q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
    else:
        q = (torch.randn(B, tq, Cc, generator=g) * 1.3).half().to(DEV)
        kv = (torch.randn(B, tkv, 2 * Cc, generator=g) * 1.3).half().to(DEV)
        k, v = kv[..., :Cc], kv[..., Cc:]

    def heads_first(x):
        return x.float().unflatten(-1, (heads, D)).transpose(1, 2)
    s = heads_first(q) @ heads_first(k).transpose(-1, -2) * D ** -0.5
    ref = (s.softmax(-1) @ heads_first(v)).transpose(1, 2).reshape(B, tq, Cc)
    got = C.attention_f16(q, k, v, heads).float()
    err = (got - ref).abs()
    assert bool((err <= ATOL + RTOL * ref.abs()).all()), f"max err {err.max().item():.3e}"
    ones = torch.ones_like(v)
    c = C.attention_f16(q, k, ones, heads)
    assert torch.equal(c, torch.ones_like(c))


@pytest.mark.parametrize("D", [16, 32, 48, 96, 128])
def test_attention_hd_other_widths_are_refused(C, D):
    heads = 2
    q = torch.zeros(1, 64, heads * D, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError):
        C.attention_f16(q, q, q, heads)


@pytest.mark.parametrize("D", WIDTHS)
def test_attention_hd_refuses_the_short_key_form_and_ignores_a_payload(C, D):
    B, tq, tkv, heads = 2, 256, 256, 2
    Cc = heads * D
    _, (qd, kd, vd) = make(55 + D, B, tq, tkv, Cc, True)
    want = C.attention_f16(qd, kd, vd, heads)
    for cfg in (1, 3, 8):                        # forms these widths do not have
        with pytest.raises(RuntimeError):
            C.attention_f16(qd, kd, vd, heads, _cfg=cfg)
    g = torch.Generator(device="cpu").manual_seed(5)
    ranges = [torch.randint(-128, 128, (n,), generator=g, dtype=torch.int8).to(DEV) for n in (4 * 1024 * 1024 + 7, 48)]
    before = [r.clone() for r in ranges]
    assert torch.equal(C.attention_f16(qd, kd, vd, heads, _prefetch=ranges), want)
    assert torch.equal(C.attention_f16(qd, kd, vd, heads, scal(S_INV), scal(ZP), _prefetch=ranges),
                       C.attention_f16(qd, kd, vd, heads, scal(S_INV), scal(ZP)))
    assert all(torch.equal(a, b) for a, b in zip(ranges, before))
    # and such a launch is no payload carrier of a PrefetchContext trace
    ctx = C.PrefetchContext(DEV)
    with ctx:
        C.attention_f16(qd, kd, vd, heads)
    assert ctx.trace == [] and ctx.att_index == 0
