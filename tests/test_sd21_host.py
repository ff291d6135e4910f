"""SD 2.x's two networks as configurations (no GPU): mixdq_amd.unet.SD21_CONFIG and mixdq_amd.text.OPENCLIP_H_CONFIG
built on the meta device -- parameter counts, layer counts, head widths, and that SD 1.5's and SDXL's did not move."""
import torch
import torch.nn as nn


def _meta(cfg):
    from mixdq_amd.unet import SDXLUNet
    with torch.device("meta"):
        return SDXLUNet(cfg)


def test_sd21_parameter_count_layers_and_heads():
    from mixdq_amd.unet import SD15_CONFIG, SD21_CONFIG, Attention, Transformer2DModel, quantizable_layers
    u = _meta(SD21_CONFIG)
    assert sum(p.numel() for p in u.parameters()) == 865_910_724           # the published figure of stable-diffusion-2-1
    q = quantizable_layers(u)
    lin = [n for n, m in q.items() if isinstance(m, nn.Linear)]
    conv = [n for n, m in q.items() if isinstance(m, nn.Conv2d)]
    # SD 1.5's 282 layers, the 32 proj_in / proj_out now Linear: 184 + 32 and 98 - 32
    assert (len(q), len(lin), len(conv)) == (282, 216, 66)
    heads = {}
    for name, m in u.named_modules():
        if isinstance(m, Attention):
            heads.setdefault(m.to_q.out_features, set()).add((m.heads, m.to_q.out_features // m.heads))
    assert heads == {320: {(5, 64)}, 640: {(10, 64)}, 1280: {(20, 64)}}
    cross = {m.to_k.in_features for m in u.modules() if isinstance(m, Attention)}
    assert cross == {320, 640, 1280, 1024}                                  # self-attention widths, and OpenCLIP-H's
    assert all(isinstance(m.proj_in, nn.Linear) for m in u.modules() if isinstance(m, Transformer2DModel))
    assert {k: v for k, v in SD21_CONFIG.items() if SD15_CONFIG[k] != v} == dict(
        head_dim=64, num_attention_heads=None, cross_attention_dim=1024, use_linear_projection=True)
    assert sum(p.numel() for p in _meta(SD15_CONFIG).parameters()) == 859_520_964


def test_example_inputs_follow_sd21():
    from mixdq_amd.quantize_sdxl import example_inputs
    from mixdq_amd.unet import SD21_CONFIG
    i = example_inputs(2, 96, "cpu", seed=1, cfg=SD21_CONFIG)
    assert tuple(i["sample"].shape) == (2, 4, 96, 96) and tuple(i["encoder_hidden_states"].shape) == (2, 77, 1024)
    assert i["added_cond_kwargs"] is None


def test_openclip_h_is_configuration_alone():
    from mixdq_amd.text import CLIP_L_CONFIG, OPENCLIP_H_CONFIG, TextEncoder, parameter_count, state_dict_names
    assert set(OPENCLIP_H_CONFIG) == set(CLIP_L_CONFIG)
    c, layers, inter = 1024, 23, 4096
    want = 49408 * c + 77 * c + layers * (4 * (c * c + c) + 4 * c + (c * inter + inter) + (inter * c + c)) + 2 * c
    assert want == 340_387_840 and parameter_count(OPENCLIP_H_CONFIG) == want
    with torch.device("meta"):
        enc = TextEncoder(OPENCLIP_H_CONFIG)
    assert sum(p.numel() for p in enc.parameters()) == want
    assert enc.heads == 16 and enc.act == "gelu" and not hasattr(enc, "text_projection")
    assert len(enc.text_model.encoder.layers) == 23                         # the 24th is never run: SD 2.x reads the penultimate
    names = dict(state_dict_names(OPENCLIP_H_CONFIG))
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == {k: tuple(v) for k, v in names.items()}
