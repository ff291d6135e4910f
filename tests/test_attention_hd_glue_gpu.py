"""SD 1.5 head widths (40, 80) through the layers above the attention kernel: the own graph's attend_out, the swapped
drop-in network (quantize_unet(..., swap_glue=True): _attention_hand_off) and HipAttnProcessor.  No attention module
of these networks may reach PyTorch's SDPA any more."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import detdata as dd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


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


def _cfg(head_dim):
    import bench
    return dict(bench.TINY_CFG, block_out_channels=(80, 160, 320), head_dim=head_dim)


def _tiny(head_dim, swap_glue):
    import bench
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet, quantizable_layers
    unet = build_unet(DEV, cfg=_cfg(head_dim))
    inputs = example_inputs(2, 32, DEV, seed=7)
    with torch.no_grad():
        unet.fp16_out = unet(**inputs)[0].float()      # the FP16 network's output, before quantization
    ckpt = calibrate(unet, [inputs])
    names = list(quantizable_layers(unet))
    quantize_unet(unet, bench.Cfg({n: 8 for n in names}, {n: 8 for n in names if n not in ("conv_in", "conv_out")}),
                  ckpt, bos=True, bos_dict=precompute_bos(unet, inputs["encoder_hidden_states"]), swap_glue=swap_glue)
    return unet, inputs


@pytest.mark.parametrize("head_dim", [40, 80])
def test_tiny_unet_fused_graph_runs_the_kernel_at_sd15_widths(C, head_dim):
    """SDXLUNet with 40- / 80-wide heads, fused graph: attend_out on the HIP kernel (self and cross), fused ==
    de-fused == hipGraph replay, and no SDPA anywhere in the fused forward."""
    import mixdq_amd.unet as U
    unet, inputs = _tiny(head_dim, False)
    attns = [m for m in unet.modules() if isinstance(m, U.Attention)]
    assert attns and all(a.to_q.out_features // a.heads == head_dim for a in attns)
    unet.set_fused(True)
    with torch.no_grad(), no_sdpa():
        fused = unet(**inputs)[0].clone()
        with U.defused():
            ref = unet(**inputs)[0].clone()
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, ref), int((fused != ref).sum())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad(), no_sdpa():
        unet(**inputs)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad(), no_sdpa():
        gout = unet(**inputs)[0]
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gout, fused)


def test_swapped_unet_at_width_40_is_the_chain_of_its_kernels(C):
    """quantize_unet(..., swap_glue=True) on the 40-wide-head network: every attention module runs the kernel
    (with the hand-off: the launch writes to_out.0's operand), output == the same network with the hand-off off ==
    the de-fused graph, and the swap undone gives the stock drop-in network's bits (SDPA's attention)."""
    import mixdq_amd.unet as U
    from mixdq_amd.nn.glue import _HipAttend, swap_glue_modules, unswap_glue_modules
    unet, inputs = _tiny(40, True)
    swapped = [m for m in unet.modules() if isinstance(m, _HipAttend)]
    assert swapped and all(m.hand_off for m in swapped)
    with torch.no_grad(), no_sdpa():
        glue = unet(**inputs)[0].clone()
    unswap_glue_modules(unet)
    with torch.no_grad():
        dropin = unet(**inputs)[0].clone()            # the stock drop-in network: PyTorch's SDPA core
    n = swap_glue_modules(unet, operands=False)
    assert n["attention"] > 0 and n["attention_handoff"] == 0
    with torch.no_grad(), no_sdpa():
        no_handoff = unet(**inputs)[0].clone()
    n = swap_glue_modules(unet)
    assert n["attention_handoff"] > 0
    with torch.no_grad(), no_sdpa():
        again = unet(**inputs)[0].clone()
        unet.set_fused(True)
        with U.defused():
            ref = unet(**inputs)[0].clone()
        unet.set_fused(False)
    assert torch.isfinite(glue).all()
    assert torch.equal(glue.view(torch.int16), again.view(torch.int16))
    assert torch.equal(glue.view(torch.int16), no_handoff.view(torch.int16))
    assert torch.equal(glue.view(torch.int16), ref.view(torch.int16)), int((glue != ref).sum())
    # within quantization noise of the drop-in network (its distance from the FP16 network), as in test_glue_gpu.py
    noise = (dropin.float() - unet.fp16_out).abs().mean()
    assert (glue.float() - dropin.float()).abs().mean() <= 1.5 * noise
    unswap_glue_modules(unet)
    with torch.no_grad():
        assert torch.equal(unet(**inputs)[0].view(torch.int16), dropin.view(torch.int16))


def test_diffusers_processor_at_width_40(C):
    from mixdq_amd.nn.glue import HipAttnProcessor, swap_glue_modules, unswap_glue_modules
    from mixdq_amd.unet import Attention
    torch.manual_seed(0)
    a = Attention(320, 768, 40).half().to(DEV)               # SD 1.5's first level: 8 heads of 40
    x = t(dd.normal_f16(81, (2, 1024, 320), 1.0))
    ctx = t(dd.normal_f16(82, (2, 77, 768), 1.0))

    class FakeDiffusersAttention(nn.Module):
        """The attributes of diffusers.models.attention_processor.Attention a processor touches."""

        def __init__(self, src, scale):
            super().__init__()
            self.to_q, self.to_k, self.to_v, self.to_out = src.to_q, src.to_k, src.to_v, src.to_out
            self.heads, self.processor, self.scale = src.heads, None, scale
            self.group_norm = self.spatial_norm = self.norm_q = self.norm_k = None
            self.norm_cross, self.residual_connection, self.rescale_output_factor = False, False, 1.0

        def set_processor(self, p):
            self.processor = p

        def forward(self, hidden_states, encoder_hidden_states=None, **kw):
            return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states, **kw)

    a_self = Attention(320, None, 40).half().to(DEV)
    stock_proc = lambda attn, hs, encoder_hidden_states=None, attention_mask=None, temb=None: "stock"   # noqa: E731
    for src, c in ((a, ctx), (a_self, None)):
        fake = FakeDiffusersAttention(src, 40 ** -0.5).to(DEV)
        fake.set_processor(stock_proc)
        assert swap_glue_modules(nn.ModuleList([fake]))["attention"] == 1
        assert isinstance(fake.processor, HipAttnProcessor)
        kv_in = x if c is None else c
        with torch.no_grad():
            want = src.to_out[0](C.attention_f16(src.to_q(x), src.to_k(kv_in), src.to_v(kv_in), src.heads))
            with no_sdpa():
                got = fake(x, c)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16))
            assert fake(x, c, attention_mask=torch.zeros(1, device=DEV)) == "stock"    # masks: the replaced processor
            fake.scale = 0.125                                                         # another scale: likewise
            assert fake(x, c) == "stock"
        unswap_glue_modules(nn.ModuleList([fake]))
        assert fake.processor is stock_proc
