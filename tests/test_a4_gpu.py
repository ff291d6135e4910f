"""4-bit activation quantizers on the INT8 kernels (MIXDQ_FLAG_A4_*, a4_kernel=True) on the MI355X: every producer
that honours the flag equals the oracle's int8 quantizer clamped to -113 bit for bit, in both rounding variants;
every other quantizing entry point refuses it; A4 modules equal the oracle's INT chain; a tiny UNet with A4
cross-attention layers and the full-size SDXL with weight_4.00 + act_7.77 keep fused == de-fused == graph replay."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_a4_host import a4_linear
from tests.test_host import Args, TINY, tiny_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A4_MAX = -113


@pytest.fixture(params=["A", "B"])
def variant(request, monkeypatch):
    import mixdq_amd._C as C_
    v = 1 if request.param == "B" else 0
    monkeypatch.setattr(C_, "FLAGS", v)
    return v


def _a4(q8):
    """The A4 reference: the oracle's int8 quantize clamped to the 4-bit range (-128 .. -113)."""
    return np.minimum(q8, A4_MAX).astype(np.int8)


def _scal(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def _f16(shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).half()


# the quantizer: zero point near the bottom of the int8 range, as a 4-bit one is after the -128 shift -- a good share
# of values lands on each side of the clamp
S_INV, ZP = 6.0, -121.0


def test_quantize_a4_dense_strided_and_bos_slice(C, oracle, variant):
    x = _f16((2, 77, 320), 1, 1.5)
    xd = x.to(DEV)
    for t, name in ((xd, "dense"), (xd[:, 1:, :], "bos slice"), (xd.transpose(1, 2), "strided"),
                    (xd[..., 3:203], "unaligned rows")):
        q4 = C.quantize_per_tensor_to_int8(t, _scal(S_INV), _scal(ZP), _abits=4).cpu().numpy()
        q8 = C.quantize_per_tensor_to_int8_vectorized(t, _scal(S_INV), _scal(ZP)).cpu().numpy()
        want8 = oracle.quantize(t.cpu().numpy(), S_INV, ZP, variant)
        assert np.array_equal(q8, want8), name
        assert np.array_equal(q4, _a4(want8)), name
        assert (q4 <= A4_MAX).all() and (q8 > A4_MAX).any(), name


def test_layernorm_quantize_slots_8_4_8(C, oracle, variant):
    x = _f16((130, 640), 2, 1.2)
    gam = (_f16((640,), 3, 0.3).float() + 1).half()
    bet = _f16((640,), 4, 0.2)
    qps = [(25.0, -3.0), (S_INV, ZP), (40.0, 11.0)]
    for rows in (130, 9000):              # one and two rows per wave
        xr = x.repeat((rows + 129) // 130, 1)[:rows].contiguous()
        outs, h = C.layernorm_quantize(xr.to(DEV), gam.to(DEV), bet.to(DEV), 1e-5,
                                       [(_scal(s), _scal(z)) for s, z in qps], want_f16=True, _abits=(8, 4, 8))
        want, want_h = oracle.layernorm_quantize(xr.numpy(), gam.numpy(), bet.numpy(), 1e-5, qps, variant)
        assert np.array_equal(h.cpu().numpy().view(np.uint16), want_h.view(np.uint16))
        assert np.array_equal(outs[0].cpu().numpy(), want[0])
        assert np.array_equal(outs[1].cpu().numpy(), _a4(want[1]))
        assert np.array_equal(outs[2].cpu().numpy(), want[2])
    for bits in ((4,), (4, 4), (8, 8, 4)):
        outs, _ = C.layernorm_quantize(x.to(DEV), gam.to(DEV), bet.to(DEV), 1e-5,
                                       [(_scal(s), _scal(z)) for s, z in qps[:len(bits)]], _abits=bits)
        want, _ = oracle.layernorm_quantize(x.numpy(), gam.numpy(), bet.numpy(), 1e-5, qps[:len(bits)], variant)
        for o, w, b in zip(outs, want, bits):
            assert np.array_equal(o.cpu().numpy(), _a4(w) if b == 4 else w), bits


def test_geglu_quantize_a4(C, oracle, variant):
    h = _f16((96, 2 * 320), 5, 2.0)
    for M in (96, 8192):                           # GELU by arithmetic / by table (from 2 Mi outputs on)
        hm = h.repeat(M // 96 + 1, 1)[:M].contiguous()
        q4, _ = C.geglu_quantize(hm.to(DEV), _scal(S_INV), _scal(ZP), _abits=4)
        want, _ = oracle.geglu_quantize(hm.numpy(), S_INV, ZP, variant)
        assert np.array_equal(q4.cpu().numpy(), _a4(want)), M


@pytest.mark.parametrize("tkv", [77, 1024])
def test_attention_a4_output(C, oracle, variant, tkv):
    """Both kernels (short-key for 77 keys, the pipelined one for 1024): the A4 output == the oracle's quantize of
    the launch's own FP16 output, clamped."""
    q = _f16((2, 256, 128), 6).to(DEV)
    k, v = _f16((2, tkv, 128), 7).to(DEV), _f16((2, tkv, 128), 8).to(DEV)
    o16 = C.attention_f16(q, k, v, 2).cpu().numpy()
    want8 = oracle.quantize(o16, 20.0, ZP, variant)
    o4 = C.attention_f16(q, k, v, 2, _scal(20.0), _scal(ZP), _abits=4).cpu().numpy()
    o8 = C.attention_f16(q, k, v, 2, _scal(20.0), _scal(ZP)).cpu().numpy()
    assert np.array_equal(o8, want8) and np.array_equal(o4, _a4(want8))
    # the prefetch entry point carries the same flag
    o4p = C.attention_f16(q, k, v, 2, _scal(20.0), _scal(ZP), _abits=4, _prefetch=[k]).cpu().numpy()
    assert np.array_equal(o4p, o4)


@pytest.mark.parametrize("wbits", [8, 4, 2])
def test_qlinear_attention_a4_output(C, oracle, variant, wbits):
    from mixdq_amd.nn.utils import pack_w2, pack_w4
    g = torch.Generator().manual_seed(wbits)
    lo = {8: -128, 4: -8, 2: -2}[wbits]
    x = torch.randint(-128, 128, (2, 64, 128), generator=g).to(torch.int8).to(DEV)
    w = torch.randint(lo, -lo, (128, 128), generator=g).to(torch.int8)
    wst = (w if wbits == 8 else pack_w4(w) if wbits == 4 else pack_w2(w)).to(DEV)
    kw = dict(_w4=wbits == 4, _w2=wbits == 2)
    sc = (torch.rand(128, generator=g) * 5e-4 + 1e-4).to(DEV)
    b0 = (torch.randn(128, generator=g) * 30).to(DEV)
    k, v = _f16((2, 77, 128), 9).to(DEV), _f16((2, 77, 128), 10).to(DEV)
    o16 = C.qlinear_attention(x, wst, sc, b0, k, v, **kw).cpu().numpy()
    want8 = oracle.quantize(o16, 20.0, ZP, variant)
    o4 = C.qlinear_attention(x, wst, sc, b0, k, v, _scal(20.0), _scal(ZP), _abits=4, **kw).cpu().numpy()
    assert np.array_equal(o4, _a4(want8))


def test_refusing_entry_points_return_unsupported(C):
    """Every other entry point that quantizes refuses each A4 bit before it looks at its operands (nothing is
    launched: the pointers may be null)."""
    lib, U = C._lib, 3     # MIXDQ_ERR_UNSUPPORTED
    vp = ctypes.c_void_p
    for f in (C.FLAG_A4_0, C.FLAG_A4_1, C.FLAG_A4_2):
        assert lib.mixdq_groupnorm_silu_quantize3(None, 64, None, None, None, ctypes.c_float(1e-5), 1, None, None,
                                                  None, None, None, None, None, None, 1, 64, 64, 8, f, None) == U
        assert lib.mixdq_qlinear_w8a8_geglu(None, None, None, None, None, None, 64, 64, 64, None, None,
                                            f | (71 << 8), None) == U
        assert lib.mixdq_qlinear_w8a8_geglu(None, None, None, None, None, None, 64, 64, 64, None, None,
                                            f, None) == U
        assert lib.mixdq_qlinear_f16in_w8a8(None, 64, None, None, None, None, None, None, None, 64, 64, 64,
                                            0, 0, 0, None, 1, f, None) == U
        assert lib.mixdq_qlinear_w8a8_ln(None, None, None, None, None, None, 64, 640, 128, None, 1, None, None,
                                         ctypes.c_float(1e-5), 1, None, None, None, None, None, f, None) == U
    # single-quantizer producers: slot 0 only
    for f in (C.FLAG_A4_1, C.FLAG_A4_2):
        assert lib.mixdq_geglu_quantize(vp(16), 8, 64, vp(16), vp(16), vp(16), None, f, None) == U
    # one width per LayerNorm quantizer
    x = torch.zeros(4, 64, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError):
        C.layernorm_quantize(x, x[0], x[0], 1e-5, [(_scal(1), _scal(0))], _abits=(8, 4))


@pytest.mark.parametrize("wbits", [8, 4, 2])
def test_a4_modules_equal_the_oracle_int_chain_and_path_a(C, oracle, wbits):
    from oracle.fakequant import quant_layer_forward
    variant = C.FLAGS & 1
    fm, m = a4_linear(wbits, K=256, N=128, seed=wbits, half=True)
    assert m.act_bits == 4 and m.valid_for_acceleration
    m = m.to(DEV)
    x = _f16((2, 77, 256), 11 + wbits, 1.5)
    with torch.no_grad():
        y = m(x.to(DEV)).cpu()
    wv = m._weight_values().cpu().numpy()
    q = _a4(oracle.quantize(x.numpy(), float(m.act_scales_inv), float(m.act_zero_points), variant))
    want = oracle.qlinear(q.reshape(-1, 256), wv, m.bias0.cpu().numpy(), m.scale.cpu().numpy(),
                          m.bias.cpu().numpy(), variant).reshape(2, 77, 128)
    assert np.array_equal(y.numpy().view(np.uint16), want.view(np.uint16))
    # Path A (qdiff simulation) at a_bits = 4 with the same fp16-rounded scales: the module tolerance
    with torch.no_grad():
        sim = quant_layer_forward(x.float(), fm.weight.float(), fm.bias.float(), m.weight_scales.cpu(),
                                  m.act_scales.cpu(), m.act_zero_points.cpu() + 128, wbits, 4)
    torch.testing.assert_close(y.float(), sim, rtol=1e-2, atol=1e-2)
    # BOS path (attn2.to_v): tokens 1.. on the kernels, token 0 the precomputed row
    m.bos = True
    m.register_buffer("bos_pre_computed", torch.full((1, 1, 128), 0.5, dtype=torch.float16, device=DEV))
    with torch.no_grad():
        yb = m(x.to(DEV)).cpu()
    assert torch.equal(yb[:, 0], torch.full((2, 128), 0.5, dtype=torch.float16))
    q1 = _a4(oracle.quantize(np.ascontiguousarray(x.numpy()[:, 1:]), float(m.act_scales_inv),
                             float(m.act_zero_points), variant))
    want_b = oracle.qlinear(q1.reshape(-1, 256), wv, m.bias0.cpu().numpy(), m.scale.cpu().numpy(),
                            m.bias.cpu().numpy(), variant).reshape(2, 76, 128)
    assert np.array_equal(yb[:, 1:].numpy().view(np.uint16), want_b.view(np.uint16))


# ------------------------------------------------------------------------------------------------- networks
def _a4_bits(n):
    """4-bit activations where MixDQ's configurations put them (attn2.to_q / to_v / to_out.0), plus ff.net.2 and
    ff.net.0.proj of some blocks (act_7.38 / act_7.84) and an attn1.to_k (a q|k|v group of mixed widths)."""
    if any(s in n for s in ("attn2.to_q", "attn2.to_v", "attn2.to_out.0")):
        return 4
    if "transformer_blocks.0.ff" in n or "transformer_blocks.1.attn1.to_k" in n:
        return 4
    return 8


def _tiny_nets(n):
    """`n` copies of a tiny UNet (head_dim 64) quantized with one calibration, mixed 8/4/2-bit weights and the
    A4 layers above under a4_kernel."""
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
    for i in range(n):
        unet = build_unet(DEV, cfg=cfg)
        names = list(quantizable_layers(unet))
        w = {"model." + nm: (8, 4, 2)[j % 3] if "attn" in nm or "ff" in nm else 8 for j, nm in enumerate(names)}
        a = {"model." + nm: _a4_bits(nm) for nm in names}
        quantize_unet(unet, Args(w, a), ckpt, bos=True, bos_dict=bos, w4_kernel=True, w2_kernel=True,
                      a4_kernel=True)
        nets.append(unet)
    return nets, inp


def _n_a4(unet):
    from mixdq_amd.nn import QuantizedLinear
    return sum(m.valid_for_acceleration and m.act_bits == 4 for m in unet.modules() if isinstance(m, QuantizedLinear))


def test_tiny_unet_a4_fused_equals_defused_and_graph(C):
    import mixdq_amd.unet as U
    (unet,), inp = _tiny_nets(1)
    assert _n_a4(unet) >= 10
    unet.set_fused(True)
    with torch.no_grad():
        fused = unet(**inp)[0].clone()
        with U.defused():
            ref = unet(**inp)[0].clone()
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, ref), int((fused != ref).sum())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        unet(**inp)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        gout = unet(**inp)[0]
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gout, fused)


def test_tiny_unet_a4_swapped_glue_equals_module_by_module(C):
    """swap_glue: the producers' INT8 operands handed on (a 4-bit consumer gets its own clamp, never an 8-bit
    operand with equal qparams) == every layer quantizing for itself == the de-fused graph."""
    import mixdq_amd.unet as U
    from mixdq_amd.nn.glue import swap_glue_modules
    (unet,), inp = _tiny_nets(1)
    assert _n_a4(unet) >= 10
    swap_glue_modules(unet, operands=False)
    with torch.no_grad():
        no_handoff = unet(**inp)[0].clone()
    n = swap_glue_modules(unet)
    assert n["operand_links"] > 0 and n["attention_handoff"] > 0
    with torch.no_grad():
        glue = unet(**inp)[0].clone()
        unet.set_fused(True)
        with U.defused():
            ref = unet(**inp)[0].clone()
        unet.set_fused(False)
    assert torch.isfinite(glue).all()
    assert torch.equal(glue, no_handoff), int((glue != no_handoff).sum())
    assert torch.equal(glue, ref), int((glue != ref).sum())


def test_full_sdxl_a4_fused_equals_defused_graph_and_batch_rows(C):
    """weight_4.00 + act_7.77, w4_kernel + w2_kernel + a4_kernel at 1024 px: all 785 layers with an activation
    quantizer run on the INT8 kernels (66 of them with the 4-bit clamp)."""
    from mixdq_amd import cfgs
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet
    from tests.test_unet_full_gpu import _check_graph
    unet = build_unet(DEV)
    inputs2 = example_inputs(2, 128, DEV, seed=7)
    ckpt = calibrate(unet, [inputs2])
    bos = precompute_bos(unet, inputs2["encoder_hidden_states"])
    quantize_unet(unet, Args(cfgs.load("weight/weight_4.00"), cfgs.load("act/act_7.77")), ckpt, bos=True,
                  bos_dict=bos, w4_kernel=True, w2_kernel=True, a4_kernel=True)
    del ckpt
    assert _n_a4(unet) == 66
    _check_graph(unet, inputs2, expect_accel=785)
    del unet
    torch.cuda.empty_cache()
