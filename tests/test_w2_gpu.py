"""Packed-W2 weights (MIXDQ_FLAG_W2) on the MI355X: every admitted tile and every Linear entry point
equals the W8 / W4 launches on the same integers bit for bit; a W2 module and a mixed 2/4/8-bit UNet
(eager, hipGraph, swapped glue, full-size SDXL) equal their W4-storage twins."""
import copy

import pytest
import torch

from tests.test_host import Args, TINY, tiny_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g, dtype=torch.int64).to(torch.int8)


def _problem(M, N, K, seed=0, bias=True):
    g = torch.Generator().manual_seed(seed + 1)
    q = _ints((N, K), -2, 2, seed)
    x = _ints((M, K), -128, 128, seed + 2)
    scale = (torch.rand(N, generator=g) * 1e-3 + 1e-4).float()
    bias0 = q.float().sum(1) * 3.0
    b = (torch.randn(N, generator=g) * 0.5).half() if bias else None
    return q, x, scale, bias0, b


def _gemm(C, x, w, scale, bias0, bias, **kw):
    v = torch.ones(w.size(0), device=DEV)
    s = torch.ones(1, device=DEV)
    return C.qlinear_w8_a8_ohalf(x, w, v, s, s, v, scale, bias0, bias, **kw)


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def test_w2_every_admitted_tile_equals_w4_w8_and_the_oracle(C, oracle):
    from mixdq_amd.nn.utils import pack_w2, pack_w4, unpack_w2
    ids = [i for i in C.IGEMM_CONFIGS if i not in C.W2_INADMISSIBLE]
    for K in (384, 320):                           # K % 128 == 0 (fast staging) and a K tail on BK = 128
        for bias in (True, False):
            q, x, scale, bias0, b = _problem(77 + K // 64, 200, K, seed=K + bias, bias=bias)
            qd, xd, sd, b0d, bd = _dev(q, x, scale, bias0, b)
            p2, p4 = pack_w2(q).to(DEV), pack_w4(q).to(DEV)
            assert torch.equal(unpack_w2(p2.cpu()), q)
            want = torch.from_numpy(oracle.qlinear(x.numpy(), unpack_w2(p2.cpu()).numpy(), bias0.numpy(),
                                                   scale.numpy(), None if b is None else b.numpy()))
            for cfg in ids:
                d8 = _gemm(C, xd, qd, sd, b0d, bd, _cfg=cfg)
                d4 = _gemm(C, xd, p4, sd, b0d, bd, _cfg=cfg, _w4=True)
                d2 = _gemm(C, xd, p2, sd, b0d, bd, _cfg=cfg, _w2=True)
                assert torch.equal(d2, d8) and torch.equal(d2, d4), (cfg, K, bias)
                assert torch.equal(d2.cpu(), want), (cfg, K, bias)
            d2 = _gemm(C, xd, p2, sd, b0d, bd, _w2=True)         # the automatic choice
            assert torch.equal(d2.cpu(), want)


def test_w2_refuses_inadmissible_tiles_bad_k_and_both_flags(C):
    from mixdq_amd.nn.utils import pack_w2, pack_w4
    q, x, scale, bias0, b = _problem(64, 160, 256)
    qd, xd, sd, b0d, bd = _dev(q, x, scale, bias0, b)
    p2 = pack_w2(q).to(DEV)
    for cfg in C.W2_INADMISSIBLE:
        with pytest.raises(RuntimeError):
            _gemm(C, xd, p2, sd, b0d, bd, _cfg=cfg, _w2=True)
    torch.cuda.synchronize()
    p = torch.zeros(160, 24, dtype=torch.int8, device=DEV)    # K = 96: not a whole 64-k piece
    with pytest.raises(RuntimeError, match="K % 64"):
        _gemm(C, _ints((64, 96), -5, 5, 4).to(DEV), p, sd, b0d, bd, _w2=True)
    with pytest.raises(RuntimeError):
        _gemm(C, xd, pack_w4(q).to(DEV), sd, b0d, bd, _w4=True, _w2=True)


def test_w2_residual_and_bos_row_map_equal_w8(C):
    from mixdq_amd.nn.utils import pack_w2
    q, x, scale, bias0, b = _problem(2 * 76, 640, 640, seed=11)
    qd, xd, sd, b0d, bd = _dev(q, x, scale, bias0, b)
    p2 = pack_w2(q).to(DEV)
    res = (torch.randn(2 * 76, 640) * 0.3).half().to(DEV)
    for div in (1, 76):
        r = res if div == 1 else res[:2].contiguous()
        d8 = _gemm(C, xd, qd, sd, b0d, bd, _residual=r, _residual_div=div)
        d2 = _gemm(C, xd, p2, sd, b0d, bd, _residual=r, _residual_div=div, _w2=True)
        assert torch.equal(d2, d8)
    out8 = torch.full((2, 77, 640), 7.0, dtype=torch.float16, device=DEV)
    out2 = out8.clone()
    _gemm(C, xd, qd, sd, b0d, bd, _out=out8, _row_map=(76, 77, 1))
    _gemm(C, xd, p2, sd, b0d, bd, _out=out2, _row_map=(76, 77, 1), _w2=True)
    assert torch.equal(out2, out8) and bool((out2[:, 0] == 7.0).all())


def test_w2_geglu_equals_w8(C):
    from mixdq_amd.nn.utils import pack_w2
    for M, N, K in ((1024, 2560, 640), (77, 640, 128)):
        q, x, scale, bias0, b = _problem(M, N, K, seed=N)
        qd, xd, sd, b0d, bd = _dev(q, x, scale, bias0, b)
        p2 = pack_w2(q).to(DEV)
        s_inv, zp = torch.tensor([0.7], device=DEV), torch.tensor([-3.0], device=DEV)
        o8 = C.qlinear_geglu(xd, qd, sd, b0d, bd, s_inv, zp)
        o2 = C.qlinear_geglu(xd, p2, sd, b0d, bd, s_inv, zp, _w2=True)
        assert torch.equal(o2, o8)
        assert C.igemm_select_id(M, N, K, w2=True, geglu=True) not in C.W2_INADMISSIBLE


def test_w2_to_q_cross_attention_launch_equals_w8(C):
    from mixdq_amd.nn.utils import pack_w2
    B, T, K, N, Tkv = 2, 128, 640, 640, 77
    q, x, scale, bias0, _ = _problem(B * T, N, K, seed=21, bias=False)
    qd, xd, sd, b0d = _dev(q, x, scale, bias0)
    xd = xd.view(B, T, K)
    g = torch.Generator().manual_seed(5)
    k = (torch.randn(B, Tkv, N, generator=g)).half().to(DEV)
    v = (torch.randn(B, Tkv, N, generator=g)).half().to(DEV)
    s_inv, zp = torch.tensor([4.0], device=DEV), torch.tensor([1.0], device=DEV)
    for quant in (False, True):
        extra = (s_inv, zp) if quant else ()
        o8 = C.qlinear_attention(xd, qd, sd, b0d, k, v, *extra)
        o2 = C.qlinear_attention(xd, pack_w2(q).to(DEV), sd, b0d, k, v, *extra, _w2=True)
        assert torch.equal(o2, o8)


def test_w2_grouped_launch_equals_w8(C):
    from mixdq_amd.nn.utils import pack_w2
    M, K = 2 * 76, 2048
    x = _ints((M, K), -128, 128, 31).to(DEV)
    members8, members2, outs8, outs2 = [], [], [], []
    for i, N in enumerate((640, 1280, 640)):
        q, _, scale, bias0, b = _problem(1, N, K, seed=40 + i, bias=i == 1)
        qd, sd, b0d, bd = _dev(q, scale, bias0, b)
        o8 = torch.empty(M, N, dtype=torch.float16, device=DEV)
        o2 = torch.empty_like(o8)
        members8.append((qd, b0d, sd, bd, o8))
        members2.append((pack_w2(q).to(DEV), b0d, sd, bd, o2))
        outs8.append(o8)
        outs2.append(o2)
    t8, t2 = C.GemmGroupTable(members8), C.GemmGroupTable(members2, wbits=2)
    assert t2.K == K and t2.w2 and not t2.w4
    for cfg in (0, 4, 35, 37, 41):
        C.qlinear_grouped(x, t8, _cfg=cfg)
        C.qlinear_grouped(x, t2, _cfg=cfg)
        for a, b_ in zip(outs2, outs8):
            assert torch.equal(a, b_), cfg
    with pytest.raises(RuntimeError):
        C.qlinear_grouped(x, t2, _cfg=56)


def test_w2_f16in_reports_unsupported_and_refuses(C):
    from mixdq_amd.nn.utils import pack_w2
    q, _, scale, bias0, _ = _problem(1, 640, 640, seed=3, bias=False)
    x = torch.randn(256, 640, device=DEV).half()
    assert not C.qlinear_f16in_supported(x, 640, 640, w2=True)
    assert not C.qlinear_f16in_wanted(x, 640, 640, w2=True)
    s_inv, zp = torch.tensor([10.0], device=DEV), torch.tensor([0.0], device=DEV)
    with pytest.raises(RuntimeError):
        C.qlinear_f16in(x, s_inv, zp, pack_w2(q).to(DEV), scale.to(DEV), bias0.to(DEV), _w2=True)


def test_w2a8_module_equals_w4_storage_and_tracks_dequantized_linear(C):
    from tests.test_w2_host import _two_bit_linear
    for K, N in ((1280, 640), (2048, 1280)):
        _, m2, _ = _two_bit_linear(w2_kernel=True, K=K, N=N, seed=K, half=True)
        fm, m4, _ = _two_bit_linear(w2_kernel=False, w4_kernel=True, K=K, N=N, seed=K, half=True)
        m2, m4 = m2.to(DEV), m4.to(DEV)
        assert m2._get_name() == "QuantizedLinearW2A8"
        x = (torch.randn(2, 77, K, generator=torch.Generator().manual_seed(K)) * 0.5).half().to(DEV)
        with torch.no_grad():
            y2, y4 = m2(x), m4(x)
            assert torch.equal(y2, y4)
            # Path A at 2-bit weights: fake-quantized activations x the dequantized 2-bit weights
            s, zp = m2.act_scales.float(), m2.act_zero_points.float()
            xq = (torch.clamp(torch.round(x.float() / s + zp), -128, 127) - zp) * s
            w = m2._weight_values().float() * m2.weight_scales[:, None]
            ref = torch.nn.functional.linear(xq, w, m2.bias.float())
        torch.testing.assert_close(y2.float(), ref, rtol=1e-2, atol=1e-2)


# ------------------------------------------------------------------ networks
def _mixed_bits(i, n):
    if "attn2.to_k" in n or "attn2.to_v" in n or "ff.net" in n or "attn2.to_out" in n or "attn2.to_q" in n:
        return 2
    if "attn1.to_k" in n:
        return 2                                    # a {8, 2, 4} q|k|v: unified to int8
    return (8, 4)[i % 2]


def _tiny_pair(swap_glue=False):
    """The same tiny UNet quantized twice with one calibration: W4 storage, and W2 storage (w2_kernel)."""
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import quantize_unet
    from mixdq_amd.unet import build_unet, quantizable_layers
    cfg = dict(TINY, block_out_channels=(64, 128, 256), head_dim=64)
    host = tiny_inputs(B=2, L=16)
    unet_c = build_unet("cpu", dtype=torch.float32, cfg=cfg)
    with torch.no_grad():
        ckpt = calibrate(unet_c, [host])
        bos = {k: v.half().to(DEV) for k, v in precompute_bos(unet_c, host["encoder_hidden_states"]).items()}
    del unet_c
    inp = dict(sample=host["sample"].half().to(DEV), timestep=host["timestep"].to(DEV),
               encoder_hidden_states=host["encoder_hidden_states"].half().to(DEV),
               added_cond_kwargs={k: v.half().to(DEV) for k, v in host["added_cond_kwargs"].items()})
    nets = []
    for w2 in (False, True):
        unet = build_unet(DEV, cfg=cfg)
        names = list(quantizable_layers(unet))
        w = {"model." + n: _mixed_bits(i, n) for i, n in enumerate(names)}
        a = {"model." + n: 8 for n in names}
        quantize_unet(unet, Args(w, a), ckpt, bos=True, bos_dict=bos, w4_kernel=True, w2_kernel=w2,
                      swap_glue=swap_glue)
        nets.append(unet)
    return nets, inp


def _n_w2(unet):
    from mixdq_amd.nn import QuantizedLinear
    return sum(bool(getattr(m, "w_packed2", False)) for m in unet.modules() if isinstance(m, QuantizedLinear))


def test_tiny_unet_w2_equals_w4_storage_eager_and_graph(C):
    (u4, u2), inp = _tiny_pair()
    assert _n_w2(u2) > 10 and _n_w2(u4) == 0
    outs = []
    for u in (u4, u2):
        u.set_fused(True)
        with torch.no_grad():
            outs.append(u(**inp)[0].clone())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[1], outs[0])
    # hipGraph replay of the W2 network
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        u2(**inp)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        gout = u2(**inp)[0]
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gout, outs[0])


def test_tiny_unet_w2_equals_w4_storage_with_swapped_glue(C):
    (u4, u2), inp = _tiny_pair(swap_glue=True)
    assert _n_w2(u2) > 10
    with torch.no_grad():
        o4, o2 = u4(**inp)[0], u2(**inp)[0]
    assert torch.isfinite(o4).all() and torch.equal(o2, o4)


def _buffer_bytes(m):
    return sum(b.numel() * b.element_size() for b in m.buffers())


def test_full_sdxl_w2_equals_w4_and_saves_memory(C):
    """1024 px, batch 1, weight_4.00 / act_7.77: the W2-storage network's output equals the W4 one's
    bit for bit, and its buffers are smaller by exactly N * K / 4 bytes per W2 layer (119 MB: the 59 2-bit
    layers with 4-bit activations stay FP16 in both, and the 2-bit members of mixed q|k|v / k|v groups are
    stored as W4 from set_fused on)."""
    from mixdq_amd import cfgs
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet
    unet = build_unet(DEV)
    inputs = example_inputs(1, 128, DEV, seed=7)
    ckpt = calibrate(unet, [inputs])
    bos = precompute_bos(unet, inputs["encoder_hidden_states"])
    twin = copy.deepcopy(unet)
    args = Args(cfgs.load("weight/weight_4.00"), cfgs.load("act/act_7.77"))
    quantize_unet(unet, args, ckpt, bos=True, bos_dict=bos, w4_kernel=True)
    quantize_unet(twin, args, ckpt, bos=True, bos_dict=bos, w4_kernel=True, w2_kernel=True)
    del ckpt
    assert _n_w2(twin) > 130
    outs = []
    for u in (unet, twin):
        u.set_fused(True)
        with torch.no_grad():
            outs.append(u(**inputs)[0].clone())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[1], outs[0])
    # every layer that keeps W2 storage after set_fused (a q|k|v or k|v group with a wider member is
    # widened there) holds N * K / 4 bytes where W4 storage holds N * K / 2
    from mixdq_amd.nn import QuantizedLinear
    expect = sum(m.out_features * m.in_features // 4 for m in twin.modules()
                 if isinstance(m, QuantizedLinear) and m.valid_for_acceleration and getattr(m, "w_packed2", False))
    saved = _buffer_bytes(unet) - _buffer_bytes(twin)
    print(f"W2 storage saves {saved / 1e6:.1f} MB of buffers")
    assert saved == expect and saved >= 110e6, (saved, expect)
