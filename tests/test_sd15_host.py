"""The SD 1.5 UNet as a network of this project (mixdq_amd.unet.SD15_CONFIG): structure, names and shapes that a
diffusers checkpoint of that network keys into, the head width per level, and the conv proj_in / proj_out wiring
against a plain-PyTorch restatement.  The SDXL defaults are pinned next to it: nothing about them may move."""
import hashlib
import json
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _meta(cfg=None):
    from mixdq_amd.unet import SDXLUNet
    with torch.device("meta"):
        return SDXLUNet(cfg)


def test_sd15_parameter_count_layers_and_names():
    from mixdq_amd.unet import SD15_CONFIG, quantizable_layers
    u = _meta(SD15_CONFIG)
    assert sum(p.numel() for p in u.parameters()) == 859_520_964
    q = quantizable_layers(u)
    lin = [n for n, m in q.items() if isinstance(m, nn.Linear)]
    conv = [n for n, m in q.items() if isinstance(m, nn.Conv2d)]
    assert (len(q), len(lin), len(conv)) == (282, 184, 98)
    assert sum(n.endswith((".proj_in", ".proj_out")) for n in conv) == 32
    assert sum(n.endswith(".conv_shortcut") for n in conv) == 14
    sd = u.state_dict()
    for name, shape in (("down_blocks.0.attentions.0.proj_in.weight", (320, 320, 1, 1)),
                        ("down_blocks.2.attentions.1.transformer_blocks.0.attn2.to_k.weight", (1280, 768)),
                        ("up_blocks.3.resnets.2.conv_shortcut.weight", (320, 640, 1, 1)),
                        ("mid_block.attentions.0.transformer_blocks.0.attn1.to_q.weight", (1280, 1280))):
        assert tuple(sd[name].shape) == shape, name
    assert not hasattr(u, "add_embedding") and not any(k.startswith("add_embedding") for k in sd)
    assert not hasattr(u.down_blocks[3], "attentions") and not hasattr(u.up_blocks[0], "attentions")
    assert len(u.down_blocks) == 4 and len(u.up_blocks) == 4
    assert not hasattr(u.down_blocks[3], "downsamplers") and not hasattr(u.up_blocks[3], "upsamplers")


def test_sd15_head_widths_per_level():
    from mixdq_amd.unet import SD15_CONFIG, Attention, head_width
    u = _meta(SD15_CONFIG)
    widths = {}
    for name, m in u.named_modules():
        if isinstance(m, Attention):
            assert m.heads == 8, name
            widths.setdefault(name.split(".attentions")[0], set()).add(m.to_q.out_features // m.heads)
    assert widths == {"down_blocks.0": {40}, "down_blocks.1": {80}, "down_blocks.2": {160}, "mid_block": {160},
                      "up_blocks.1": {160}, "up_blocks.2": {80}, "up_blocks.3": {40}}
    assert [head_width(SD15_CONFIG, c) for c in SD15_CONFIG["block_out_channels"]] == [40, 80, 160, 160]
    assert head_width(dict(head_dim=64), 1280) == 64              # a head WIDTH keeps working


def test_sdxl_defaults_did_not_move():
    from mixdq_amd.unet import SDXL_CONFIG, quantizable_layers
    u = _meta()
    assert sum(p.numel() for p in u.parameters()) == 2_567_463_684
    names = list(quantizable_layers(u))
    with open(os.path.join(ROOT, "mixdq_amd", "cfgs", "bitwidths.json")) as f:
        d = json.load(f)
    assert len(names) == d["n_layers"] == 794
    assert hashlib.sha256("\n".join(names).encode()).hexdigest() == d["names_sha256"]
    assert hasattr(u, "add_embedding")
    assert isinstance(u.mid_block.attentions[0].proj_in, nn.Linear)
    assert SDXL_CONFIG["head_dim"] == 64 and "num_attention_heads" not in SDXL_CONFIG


def test_example_inputs_follow_the_config():
    from mixdq_amd.quantize_sdxl import example_inputs
    from mixdq_amd.unet import SD15_CONFIG
    i = example_inputs(2, 64, "cpu", seed=1, cfg=SD15_CONFIG)
    assert tuple(i["sample"].shape) == (2, 4, 64, 64) and tuple(i["encoder_hidden_states"].shape) == (2, 77, 768)
    assert i["added_cond_kwargs"] is None
    j = example_inputs(2, 64, "cpu", seed=1)
    assert tuple(j["encoder_hidden_states"].shape) == (2, 77, 2048) and "time_ids" in j["added_cond_kwargs"]
    assert torch.equal(i["sample"], j["sample"])


# ---- a plain-PyTorch restatement of the SD 1.5 graph (diffusers' UNet2DConditionModel with
# use_linear_projection False), reading the network's own parameters by name --------------------------------------
def _ref_resnet(r, x, temb):
    h = r.conv1(F.silu(r.norm1(x)))
    h = h + r.time_emb_proj(F.silu(temb))[:, :, None, None]
    h = r.conv2(F.silu(r.norm2(h)))
    return (x if r.conv_shortcut is None else r.conv_shortcut(x)) + h


def _ref_attn(a, x, ctx):
    ctx = x if ctx is None else ctx
    B, T, C = x.shape
    h = a.heads

    def split(t):
        return t.reshape(B, -1, h, C // h).permute(0, 2, 1, 3)
    q, k, v = split(a.to_q(x)), split(a.to_k(ctx)), split(a.to_v(ctx))
    p = torch.softmax(q @ k.transpose(-1, -2) * (C // h) ** -0.5, dim=-1)
    return a.to_out[0]((p @ v).permute(0, 2, 1, 3).reshape(B, T, C))


def _ref_transformer(t, x, ctx):
    B, C, H, W = x.shape
    res = x
    h = F.group_norm(x, t.norm.num_groups, t.norm.weight, t.norm.bias, t.norm.eps)
    h = F.conv2d(h, t.proj_in.weight, t.proj_in.bias)                      # norm -> conv -> tokens
    h = h.permute(0, 2, 3, 1).reshape(B, H * W, C)
    for b in t.transformer_blocks:
        h = h + _ref_attn(b.attn1, b.norm1(h), None)
        h = h + _ref_attn(b.attn2, b.norm2(h), ctx)
        a, gate = b.ff.net[0].proj(b.norm3(h)).chunk(2, dim=-1)
        h = h + b.ff.net[2](a * F.gelu(gate))
    h = h.reshape(B, H, W, C).permute(0, 3, 1, 2)
    return F.conv2d(h, t.proj_out.weight, t.proj_out.bias) + res           # tokens -> conv -> + residual


def _ref_unet(u, sample, timestep, ctx):
    from mixdq_amd.unet import sinusoidal_embedding
    B = sample.shape[0]
    t = torch.as_tensor(timestep, dtype=torch.float32).reshape(-1).expand(B)
    emb = u.time_embedding(sinusoidal_embedding(t, u.cfg["block_out_channels"][0]).to(sample.dtype))
    x = u.conv_in(sample)
    skips = [x]
    for blk in u.down_blocks:
        for i, r in enumerate(blk.resnets):
            x = _ref_resnet(r, x, emb)
            if hasattr(blk, "attentions"):
                x = _ref_transformer(blk.attentions[i], x, ctx)
            skips.append(x)
        if hasattr(blk, "downsamplers"):
            x = blk.downsamplers[0].conv(x)
            skips.append(x)
    x = _ref_resnet(u.mid_block.resnets[0], x, emb)
    x = _ref_transformer(u.mid_block.attentions[0], x, ctx)
    x = _ref_resnet(u.mid_block.resnets[1], x, emb)
    for blk in u.up_blocks:
        for i, r in enumerate(blk.resnets):
            x = _ref_resnet(r, torch.cat([x, skips.pop()], dim=1), emb)
            if hasattr(blk, "attentions"):
                x = _ref_transformer(blk.attentions[i], x, ctx)
        if hasattr(blk, "upsamplers"):
            x = blk.upsamplers[0].conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))
    assert not skips
    return u.conv_out(F.silu(u.conv_norm_out(x)))


def test_reduced_sd15_network_equals_a_plain_restatement():
    """Same topology as SD 1.5 (four levels, depths 1 / 1 / 1 / 0, mid 1, 8 heads per level, conv projections, no
    addition embedding) at small channel counts, CPU, FP32."""
    from mixdq_amd.quantize_sdxl import example_inputs
    from mixdq_amd.unet import SD15_CONFIG, SDXLUNet, init_synthetic_weights
    cfg = dict(SD15_CONFIG, block_out_channels=(32, 64, 128, 128), cross_attention_dim=48, time_embed_dim=64,
               norm_num_groups=8)
    u = init_synthetic_weights(SDXLUNet(cfg), std=0.05).eval()
    assert isinstance(u.down_blocks[0].attentions[0].proj_in, nn.Conv2d)
    inp = example_inputs(2, 16, "cpu", seed=3, cfg=cfg)
    sample, ctx = inp["sample"].float(), inp["encoder_hidden_states"].float()
    with torch.no_grad():
        got = u(sample, inp["timestep"], ctx, None)[0]
        also = u(sample, inp["timestep"], ctx)[0]                       # added_cond_kwargs may be omitted
        want = _ref_unet(u, sample, inp["timestep"], ctx)
    assert torch.equal(got, also)
    assert got.shape == (2, 4, 16, 16) and torch.isfinite(got).all() and float(got.abs().max()) > 0
    # FP32 on both sides; SDPA and the explicit softmax differ in summation order only
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-5), float((got - want).abs().max())
    # ... and the projections matter: a network whose proj_out were skipped would not pass
    with torch.no_grad():
        u.mid_block.attentions[0].proj_out.weight.mul_(2.0)
        assert not torch.allclose(u(sample, inp["timestep"], ctx)[0], want, rtol=1e-4, atol=1e-5)
