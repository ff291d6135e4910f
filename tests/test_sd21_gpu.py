"""mixdq_amd.unet.SD21_CONFIG at reduced width on the GPU (channels 64 / 128 / 256 / 256: 1 / 2 / 4 / 4 heads of 64
columns, Linear proj_in / proj_out, and the full cross_attention_dim of 1024), uniform W8A8 + BOS, through the forms
tests/test_sd15_gpu.py takes the SD 1.5 network through, with its requirements: fused == de-fused and hipGraph replay
== eager bit for bit, no attention module reaches PyTorch's SDPA, quantize_unet swaps every layer, swap_glue == the
de-fused graph, unswap restores the drop-in bits, and the swapped network lies within 1.5 x the drop-in network's own
distance from the FP16 network."""
import pytest
import torch
import torch.nn as nn

from tests.test_sd15_gpu import _bits_equal, _Cfg, _replay, _slice_inputs, no_sdpa

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LATENT = 32


@pytest.fixture(scope="module")
def net(C):
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import SD21_CONFIG, build_unet, quantizable_layers
    cfg = dict(SD21_CONFIG, block_out_channels=(64, 128, 256, 256))
    unet = build_unet(DEV, cfg=cfg)
    inputs2 = example_inputs(2, LATENT, DEV, seed=7, cfg=cfg)
    assert inputs2["added_cond_kwargs"] is None and inputs2["encoder_hidden_states"].shape == (2, 77, 1024)
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


def test_sd21_modules_after_the_swap(net):
    import mixdq_amd.unet as U
    from mixdq_amd.nn import QuantizedConv2d, QuantizedLinear
    unet, _, _ = net
    assert not any(type(m) in (nn.Linear, nn.Conv2d) for m in unet.modules())
    tr = [m for m in unet.modules() if isinstance(m, U.Transformer2DModel)]
    assert len(tr) == 16
    for m in tr:
        for p in (m.proj_in, m.proj_out):
            assert isinstance(p, QuantizedLinear) and p.valid_for_acceleration
    attn = [a for a in unet.modules() if isinstance(a, U.Attention)]
    assert {a.to_q.out_features // a.heads for a in attn} == {64} and {a.heads for a in attn} == {1, 2, 4}
    cross = [a for a in attn if a.to_k.in_features == 1024]
    assert len(cross) == 16 and all(a.to_k.valid_for_acceleration and a.to_v.valid_for_acceleration for a in cross)
    assert sum(isinstance(m, QuantizedLinear) for m in unet.modules()) == 216
    assert sum(isinstance(m, QuantizedConv2d) for m in unet.modules()) == 66


def test_sd21_fused_graph(net):
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
        print(f"SD 2.1 (reduced) fused graph, W8A8: mean |quantized - FP16| {d:.6f}, mean |FP16| "
              f"{fp16.abs().mean().item():.6f}")
        assert d == d and d < float("inf")
    finally:
        unet.set_fused(False)


def test_sd21_swap_glue(net):
    import mixdq_amd.unet as U
    from mixdq_amd.nn.glue import _HipAttend, swap_glue_modules, unswap_glue_modules
    unet, inputs2, fp16 = net
    with torch.no_grad():
        dropin = unet(**inputs2)[0].clone()
    try:
        n = swap_glue_modules(unet)
        assert n["attention"] == 32 and n["attention_handoff"] == 32 and n["operand_links"] > 0, n
        assert all(isinstance(m, _HipAttend) for m in unet.modules() if isinstance(m, U.Attention))
        with torch.no_grad(), no_sdpa():
            glue2 = unet(**inputs2)[0].clone()
            _bits_equal(_replay(unet, inputs2), glue2, "swap_glue: hipGraph replay != eager")
        assert torch.isfinite(glue2).all()
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
    print(f"SD 2.1 (reduced) W8A8: mean |drop-in - FP16| {noise:.6f}, mean |swap_glue - drop-in| {dist:.6f}")
    assert noise == noise and noise < float("inf") and torch.isfinite(dropin).all()
    assert dist <= 1.5 * noise, (dist, noise)
