"""`quantize_unet(..., swap_glue=True)` (mixdq_amd/nn/glue.py) on the REAL graph: the 794-layer SDXL UNet at 1024 px
(latent 128), batch 2, built and calibrated as in tests/test_unet_full_gpu.py.  The tiny-UNet test of the same
properties (tests/test_glue_gpu.py) cannot reach what only the full size has: 4096-token self-attention through the
packed q | k | v GEMM, kept 77-row BOS buffers at 1280 channels, the one-launch to_q + cross-attention at 4096 rows,
the 10240-wide GEGLU, and the operand hand-off at every OPERAND_PAIRS link.  Bit-level, not tolerance:

  * swap_glue with operand hand-off == without == the fused graph's de-fused reference (mixdq_amd.unet.defused);
    the fused graph is pinned to that reference, so this ties the swapped network to the benchmarked one;
  * row 0 of the batch-2 run == the batch-1 run; hipGraph replay == eager for both shapes, both graphs cached;
  * unswap_glue_modules gives the drop-in network's bits back.

The one leg that is a tolerance: PyTorch's SDPA kept (`attention=False`) rounds differently from
mixdq_attention_f16, so it is bounded by the quantization noise of the drop-in network, as in the tiny test."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Cfg:
    def __init__(self, w, a):
        self.w_config, self.a_config = w, a


def _slice_inputs(inp, lo, hi):
    return dict(sample=inp["sample"][lo:hi].contiguous(), timestep=inp["timestep"],
                encoder_hidden_states=inp["encoder_hidden_states"][lo:hi].contiguous(),
                added_cond_kwargs={k: v[lo:hi].contiguous() for k, v in inp["added_cond_kwargs"].items()})


def _build(w_name, a_name, **quantize_kw):
    """(unet, batch-2 inputs, the FP16 network's output on them): the FP16 forward runs before quantize_unet."""
    from mixdq_amd import cfgs
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet
    unet = build_unet(DEV)
    inputs2 = example_inputs(2, 128, DEV, seed=7)
    with torch.no_grad():
        fp16 = unet(**inputs2)[0].float()
    ckpt = calibrate(unet, [inputs2])
    bos = precompute_bos(unet, inputs2["encoder_hidden_states"])
    quantize_unet(unet, _Cfg(cfgs.load(w_name), cfgs.load(a_name)), ckpt, bos=True, bos_dict=bos, **quantize_kw)
    del ckpt
    return unet, inputs2, fp16


def _defused_reference(unet, inputs):
    import mixdq_amd.unet as U
    unet.set_fused(True)
    try:
        with torch.no_grad(), U.defused():
            return unet(**inputs)[0].clone()
    finally:
        unet.set_fused(False)


def _replays(unet, *inputs):
    """hipGraph replay of each input set in turn (one graph per shape, captured on first use)."""
    from mixdq_amd.quantize_sdxl import hip_graph_opt
    eager = unet.forward
    hip_graph_opt(unet)
    try:
        with torch.no_grad():
            outs = [unet(**inp)[0].clone() for inp in inputs]
        cached = len(unet.forward._cached)
    finally:
        unet.forward = eager
    return outs, cached


def _bits_equal(a, b, what):
    d = (a.float() - b.float()).abs()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), \
        f"{what}: {int((d > 0).sum())} of {d.numel()} elements differ, max {d.max().item():.4g}"


def test_full_unet_w8a8_swap_glue_equals_defused_graph(C):
    """uniform_8 + act_8.00 + BOS (the bench configuration) with the glue swapped as `dropin_glue*` of bench.py."""
    import bench
    import mixdq_amd.unet as U
    from mixdq_amd.nn.glue import _BOS_BUFS, _HipAttend, swap_glue_modules, unswap_glue_modules
    unet, inputs2, fp16 = _build("weight/uniform_8", "act/act_8.00")
    inputs1 = _slice_inputs(inputs2, 0, 1)
    # what the swap must find, counted on the stock network
    mods = list(unet.modules())
    n_res = sum(type(m) is U.ResnetBlock2D for m in mods)
    n_tb = sum(type(m) is U.BasicTransformerBlock for m in mods)
    want = dict(groupnorm=sum(type(m) is nn.GroupNorm for m in mods), silu_folded=2 * n_res + 1,
                layernorm=sum(type(m) is nn.LayerNorm for m in mods), geglu=sum(type(m) is U.GEGLU for m in mods),
                attention=sum(isinstance(m, U.Attention) for m in mods))
    assert n_res > 0 and n_tb > 0 and want["attention"] == 2 * n_tb
    with torch.no_grad():
        dropin = unet(**inputs2)[0].clone()

    n = swap_glue_modules(unet, operands=False)         # every layer runs its own quantize launch
    assert n == dict(want, operand_links=0, attention_handoff=0), n
    with torch.no_grad():
        no_handoff = unet(**inputs2)[0].clone()
    k_no = bench.count_kernels(lambda: unet(**inputs2), torch.device(DEV))
    n = swap_glue_modules(unet)                          # ... and the producers' operands handed on (the default)
    assert n["operand_links"] > 0 and n["attention_handoff"] == want["attention"] and n["groupnorm"] == 0, n
    with torch.no_grad():
        glue2 = unet(**inputs2)[0].clone()
        glue1 = unet(**inputs1)[0].clone()
    k_yes = bench.count_kernels(lambda: unet(**inputs2), torch.device(DEV))
    print(f"swap_glue at 1024 px, batch 2: {k_no} kernels without operand hand-off, {k_yes} with; "
          f"{n_tb} transformer blocks, {n_res} ResNet blocks")
    assert torch.isfinite(glue2).all()
    _bits_equal(glue2, no_handoff, "operand hand-off != module by module")
    _bits_equal(glue2[:1], glue1, "row 0 of the batch-2 run != the batch-1 run")
    # per transformer block at least the quantize launches of q | k | v, to_q, the GEGLU projection, net.2, two
    # to_out.0, one of attn2.to_k / to_v, two of the self-attention's projections and one of to_q + cross-attention
    assert k_no is not None and k_yes is not None and k_no - k_yes >= 12 * n_tb, (k_no, k_yes)

    attns = [m for m in unet.modules() if isinstance(m, _HipAttend)]
    selfs = [a for a in attns if a.to_k.in_features == a.to_q.in_features]
    cross = [a for a in attns if a.to_k.in_features != a.to_q.in_features]
    assert len(selfs) == len(cross) == n_tb
    for a in selfs:                                      # the q | k | v pack, valid for the layers as they are
        assert U._pack_valid(a.__dict__.get("_qkv"), [a.to_q, a.to_k, a.to_v])
    dev = torch.device(DEV)
    for a in cross:                                      # a kept BOS buffer per shape run, row 0 = the BOS row
        for layer in (a.to_k, a.to_v):
            bufs = layer.__dict__.get(_BOS_BUFS, {})
            for B in (2, 1):
                buf = bufs[(B, 77, dev)][0]
                assert buf.shape == (B, 77, layer.out_features)
                assert torch.equal(buf[:, :1], layer.bos_pre_computed.expand(B, 1, -1))

    _bits_equal(glue2, _defused_reference(unet, inputs2), "swap_glue != the de-fused reference of the fused graph")
    (g2, g1, g2b), cached = _replays(unet, inputs2, inputs1, inputs2)
    assert cached == 2
    _bits_equal(g2, glue2, "hipGraph replay, batch 2")
    _bits_equal(g1, glue1, "hipGraph replay, batch 1")
    _bits_equal(g2b, glue2, "hipGraph replay, batch 2 after batch 1")

    unswap_glue_modules(unet)
    with torch.no_grad():
        _bits_equal(unet(**inputs2)[0], dropin, "unswapped != the drop-in network")
    # PyTorch's SDPA kept (bench.py's dropin_glue_torch_sdpa): other rounding in the attention core, so within the
    # quantization noise of the drop-in network rather than bit for bit
    n = swap_glue_modules(unet, attention=False)
    assert n["attention"] == 0 and n["groupnorm"] == want["groupnorm"]
    with torch.no_grad():
        sdpa = unet(**inputs2)[0].float()
    noise = (dropin.float() - fp16).abs().mean().item()
    d_sdpa = (sdpa - glue2.float()).abs().mean().item()
    print(f"torch SDPA leg: mean |sdpa - glue| {d_sdpa:.5f}, drop-in noise {noise:.5f}")
    assert torch.isfinite(sdpa).all() and d_sdpa <= 1.5 * noise, (d_sdpa, noise)
    del unet
    torch.cuda.empty_cache()


def test_full_unet_mixed_widths_swap_glue_equals_defused_graph(C):
    """weight_4.00 + act_7.77 with w4_kernel + w2_kernel + a4_kernel and swap_glue=True: the 4-bit-clamp hand-offs
    (LayerNorm -> 4-bit to_q / to_k / to_v, GEGLU -> 4-bit net.2, the attention writing a 4-bit to_out.0 operand;
    a GroupNorm hands on to 8-bit consumers only) at full size == the de-fused reference; replay == eager."""
    from mixdq_amd.nn.glue import _CONSUMERS, HipGroupNorm, HipLayerNorm, _HipAttend, _HipGEGLU, _abits
    unet, inputs2, _ = _build("weight/weight_4.00", "act/act_7.77", w4_kernel=True, w2_kernel=True, a4_kernel=True,
                              swap_glue=True)
    a4 = lambda m: bool(getattr(m, "valid_for_acceleration", False) and _abits(m) == 4)    # noqa: E731
    prods = [m for m in unet.modules() if isinstance(m, (HipLayerNorm, _HipGEGLU))]
    n_ln4 = sum(a4(c) for m in prods if isinstance(m, HipLayerNorm) for c in m.__dict__.get(_CONSUMERS, ()))
    n_gg4 = sum(a4(c) for m in prods if isinstance(m, _HipGEGLU) for c in m.__dict__.get(_CONSUMERS, ()))
    n_out4 = sum(a4(m.to_out[0]) for m in unet.modules() if isinstance(m, _HipAttend))
    n_gn4 = sum(a4(c) for m in unet.modules() if isinstance(m, HipGroupNorm) for c in m.__dict__.get(_CONSUMERS, ()))
    print(f"4-bit consumers: {n_ln4} behind LayerNorms, {n_gg4} behind GEGLUs, {n_out4} to_out.0, {n_gn4} behind GroupNorms")
    assert n_ln4 + n_gg4 + n_out4 > 0
    with torch.no_grad():
        glue2 = unet(**inputs2)[0].clone()
    assert torch.isfinite(glue2).all()
    _bits_equal(glue2, _defused_reference(unet, inputs2), "swap_glue != the de-fused reference of the fused graph")
    (g1, g2), _ = _replays(unet, inputs2, inputs2)
    _bits_equal(g1, glue2, "hipGraph replay")
    _bits_equal(g2, glue2, "hipGraph replay (again)")
    del unet
    torch.cuda.empty_cache()
