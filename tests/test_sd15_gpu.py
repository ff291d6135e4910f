"""The full-size SD 1.5 UNet (mixdq_amd.unet.SD15_CONFIG: 282 layers, heads of 40 / 80 / 160 columns, conv proj_in /
proj_out, no addition embedding) at 512 px (latent 64), uniform W8A8 + BOS, through the three forms this project
gives a network: the fused graph, its de-fused reference, and quantize_unet(..., swap_glue=True).

Bit-level wherever the arithmetic is the same: fused == de-fused, hipGraph replay == eager, row 0 of the batch-2 run
== the batch-1 run, swap_glue == the de-fused graph == swap_glue with the operand hand-off off, unswap == the drop-in
network.  No attention module may reach PyTorch's SDPA.  The one tolerance is the bound
tests/test_attention_hd_glue_gpu.py already uses, measured on the drop-in path and not on the code under test: the
swapped network lies within 1.5 x the drop-in network's own distance from the FP16 network.  The quantized networks'
distance from FP16 is printed (DESIGN.md section 3.20 quotes it), and only asserted finite."""
import contextlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@contextlib.contextmanager
def no_sdpa():
    """F.scaled_dot_product_attention replaced by a stub that raises."""
    saved = F.scaled_dot_product_attention

    def stub(*a, **k):
        raise AssertionError("an attention module reached F.scaled_dot_product_attention")
    F.scaled_dot_product_attention = stub
    try:
        yield
    finally:
        F.scaled_dot_product_attention = saved


class _Cfg:
    def __init__(self, w, a):
        self.w_config, self.a_config = w, a


def _slice_inputs(inp, lo, hi):
    return dict(sample=inp["sample"][lo:hi].contiguous(), timestep=inp["timestep"],
                encoder_hidden_states=inp["encoder_hidden_states"][lo:hi].contiguous(), added_cond_kwargs=None)


def _bits_equal(a, b, what):
    d = (a.float() - b.float()).abs()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), \
        f"{what}: {int((d > 0).sum())} of {d.numel()} elements differ, max {d.max().item():.4g}"


@pytest.fixture(scope="module")
def net(C):
    """(the drop-in quantized SD 1.5 network, batch-2 inputs, the FP16 network's output on them)."""
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import SD15_CONFIG, build_unet, quantizable_layers
    unet = build_unet(DEV, cfg=SD15_CONFIG)
    inputs2 = example_inputs(2, 64, DEV, seed=7, cfg=SD15_CONFIG)
    assert inputs2["added_cond_kwargs"] is None and inputs2["encoder_hidden_states"].shape == (2, 77, 768)
    with torch.no_grad():
        fp16 = unet(**inputs2)[0].float()
    ckpt = calibrate(unet, [inputs2])
    names = list(quantizable_layers(unet))
    assert len(names) == 282
    quantize_unet(unet, _Cfg({n: 8 for n in names}, {n: 8 for n in names if n not in ("conv_in", "conv_out")}),
                  ckpt, bos=True, bos_dict=precompute_bos(unet, inputs2["encoder_hidden_states"]))
    yield unet, inputs2, fp16
    del unet
    torch.cuda.empty_cache()


def _replay(unet, inputs):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        unet(**inputs)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        out = unet(**inputs)[0]
    g.replay()
    torch.cuda.synchronize()
    return out.clone()


def test_sd15_modules_after_the_swap(net):
    """Every Linear / Conv2d is a quantized layer; the conv proj_in / proj_out are W8A8 QuantizedConv2d; every
    attention module has 8 heads of its level's width."""
    import mixdq_amd.unet as U
    from mixdq_amd.nn import QuantizedConv2d, QuantizedLinear
    unet, _, _ = net
    assert not any(type(m) in (nn.Linear, nn.Conv2d) for m in unet.modules())
    tr = [m for m in unet.modules() if isinstance(m, U.Transformer2DModel)]
    assert len(tr) == 16
    for m in tr:
        for p in (m.proj_in, m.proj_out):
            assert isinstance(p, QuantizedConv2d) and p.valid_for_acceleration and p.kernel_size == (1, 1)
    widths = sorted({a.to_q.out_features // a.heads for a in unet.modules() if isinstance(a, U.Attention)})
    assert widths == [40, 80, 160]
    assert sum(isinstance(m, QuantizedLinear) for m in unet.modules()) == 184
    assert sum(isinstance(m, QuantizedConv2d) for m in unet.modules()) == 98


def test_sd15_fused_graph(net):
    """fused == de-fused bit for bit, hipGraph replay == eager, no SDPA, batch 1 and 2; row 0 of the batch-2 run ==
    the batch-1 run of that image."""
    import mixdq_amd.unet as U
    unet, inputs2, fp16 = net
    inputs1 = _slice_inputs(inputs2, 0, 1)
    unet.set_fused(True)
    try:
        outs = {}
        for B, inp in ((2, inputs2), (1, inputs1)):
            with torch.no_grad(), no_sdpa():
                fused = unet(**inp)[0].clone()
                with U.defused():
                    ref = unet(**inp)[0].clone()
                assert torch.isfinite(fused).all()
                _bits_equal(fused, ref, f"fused != de-fused, batch {B}")
                _bits_equal(_replay(unet, inp), fused, f"hipGraph replay != eager, batch {B}")
            outs[B] = fused
        _bits_equal(outs[2][:1], outs[1], "row 0 of the batch-2 run != the batch-1 run")
        d = (outs[2].float() - fp16).abs().mean().item()
        print(f"SD 1.5 fused graph, W8A8: mean |quantized - FP16| {d:.6f}, mean |FP16| {fp16.abs().mean().item():.6f}")
        assert d == d and d < float("inf")
    finally:
        unet.set_fused(False)


def test_sd15_swap_glue(net):
    """quantize_unet's glue swap on the SD 1.5 network: == the de-fused graph == hand-off off, the GroupNorm in front
    of a conv proj_in hands its operand on, unswap restores the drop-in bits, and the distance from the drop-in
    network is within 1.5 x that network's own distance from FP16."""
    import mixdq_amd.unet as U
    from mixdq_amd.nn.glue import (_CONSUMERS, HipGroupNorm, _HipAttend, swap_glue_modules, tagged_operand,
                                   unswap_glue_modules)
    unet, inputs2, fp16 = net
    inputs1 = _slice_inputs(inputs2, 0, 1)
    with torch.no_grad():
        dropin = unet(**inputs2)[0].clone()
    try:
        n = swap_glue_modules(unet, operands=False)
        n_attn = sum(isinstance(m, U.Attention) for m in unet.modules())
        assert n["attention"] == n_attn == 32 and n["attention_handoff"] == 0 and n["operand_links"] == 0, n
        assert all(isinstance(m, _HipAttend) for m in unet.modules() if isinstance(m, U.Attention))
        with torch.no_grad(), no_sdpa():
            no_handoff = unet(**inputs2)[0].clone()
        n = swap_glue_modules(unet)
        assert n["attention_handoff"] == 32 and n["operand_links"] > 0, n
        # the GroupNorm of every Transformer2DModel is linked to its conv proj_in, and the operand arrives
        tr = [m for m in unet.modules() if isinstance(m, U.Transformer2DModel)]
        for m in tr:
            assert isinstance(m.norm, HipGroupNorm) and m.norm.__dict__.get(_CONSUMERS) == (m.proj_in,)
        t0 = tr[0]
        x = torch.randn(1, t0.proj_in.in_channels, 64, 64, device=DEV, dtype=torch.float16
                        ).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            y = t0.norm(x)
            q = tagged_operand(y, t0.proj_in)
            assert q is not None and q.dtype == torch.int8
            assert torch.equal(q, _quant_for(y, t0.proj_in))         # the bits proj_in's own quantize launch gives
        with torch.no_grad(), no_sdpa():
            glue2 = unet(**inputs2)[0].clone()
            glue1 = unet(**inputs1)[0].clone()
            _bits_equal(_replay(unet, inputs2), glue2, "swap_glue: hipGraph replay != eager")
        assert torch.isfinite(glue2).all()
        _bits_equal(glue2, no_handoff, "operand hand-off != module by module")
        _bits_equal(glue2[:1], glue1, "swap_glue: row 0 of the batch-2 run != the batch-1 run")
        unet.set_fused(True)
        try:
            with torch.no_grad(), no_sdpa(), U.defused():
                ref = unet(**inputs2)[0].clone()
        finally:
            unet.set_fused(False)
        _bits_equal(glue2, ref, "swap_glue != the de-fused reference of the fused graph")
    finally:
        unswap_glue_modules(unet)
    with torch.no_grad():
        _bits_equal(unet(**inputs2)[0], dropin, "unswapped != the drop-in network")
    noise = (dropin.float() - fp16).abs().mean().item()
    dist = (glue2.float() - dropin.float()).abs().mean().item()
    print(f"SD 1.5 W8A8: mean |drop-in - FP16| {noise:.6f}, mean |swap_glue - drop-in| {dist:.6f}, "
          f"mean |swap_glue - FP16| {(glue2.float() - fp16).abs().mean().item():.6f}")
    assert noise == noise and noise < float("inf") and torch.isfinite(dropin).all()
    assert dist <= 1.5 * noise, (dist, noise)


def _quant_for(y, layer):
    from mixdq_amd.nn.Conv2d import quant_op
    return quant_op(y, layer.act_scales_inv, layer.act_zero_points)
