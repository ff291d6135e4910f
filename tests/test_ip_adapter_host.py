"""IP-Adapter on the CPU: the adapter's parameter names and counts (the published checkpoint's layout), IPAdapter.kv's
column slices against per-layer F.linear, the cross-attention with image keys against a hand-written decoupled block,
and what SDXLUNet.forward(ip=) and the Sampler refuse.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from mixdq_amd.ip_adapter import IPState, build_ip_adapter
from mixdq_amd.unet import SD15_CONFIG, SDXL_CONFIG, Attention, build_unet

TINY = dict(block_out_channels=(32, 64), transformer_layers_per_block=(1, 1), mid_transformer_layers=1, head_dim=16,
            cross_attention_dim=48, time_embed_dim=64, addition_time_embed_dim=8,
            projection_class_embeddings_input_dim=8 * 6 + 40, norm_num_groups=8, layers_per_block=1)


@pytest.mark.parametrize("cfg,layers,cross", [(SDXL_CONFIG, 70, 2048), (SD15_CONFIG, 16, 768)], ids=["sdxl", "sd15"])
def test_parameter_names_and_counts(cfg, layers, cross):
    ad = build_ip_adapter(cfg, 1024, num_tokens=4, device="meta")
    sd = ad.state_dict()
    assert len(ad.dims) == layers and len(sd) == 4 + 2 * layers
    assert tuple(sd["image_proj.proj.weight"].shape) == (4 * cross, 1024) and tuple(sd["image_proj.norm.weight"].shape) == (cross,)
    for n, c in enumerate(ad.dims):                                     # i = 2 n + 1, bias-free
        for name in ("to_k_ip", "to_v_ip"):
            assert tuple(sd[f"ip_adapter.{2 * n + 1}.{name}.weight"].shape) == (c, cross)
            assert f"ip_adapter.{2 * n + 1}.{name}.bias" not in sd
    assert ad.offsets[-1] + 2 * ad.dims[-1] == 2 * sum(ad.dims)


def test_kv_slices_are_the_per_layer_projections():
    ad = build_ip_adapter(TINY, 24, num_tokens=4, dtype=torch.float32)
    tok = ad.tokens(torch.randn(3, 24, generator=torch.Generator().manual_seed(1)))
    assert tuple(tok.shape) == (3, 4, 48)
    kv = ad.kv(tok)
    for n, (c, off) in enumerate(zip(ad.dims, ad.offsets)):
        layer = ad.ip_adapter[str(2 * n + 1)]
        torch.testing.assert_close(kv[..., off:off + c], F.linear(tok, layer.to_k_ip.weight), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(kv[..., off + c:off + 2 * c], F.linear(tok, layer.to_v_ip.weight), rtol=1e-5, atol=1e-5)
    w = ad.stacked_weight()
    with torch.no_grad():
        ad.ip_adapter["1"].to_k_ip.weight.mul_(2.0)                    # an in-place write: same tensor, new rows
    assert ad.stacked_weight().data_ptr() == w.data_ptr()
    torch.testing.assert_close(w[:ad.dims[0]], ad.ip_adapter["1"].to_k_ip.weight)


def _attn(q, k, v, heads):
    B, T, C = q.shape
    sp = lambda x: x.reshape(B, -1, heads, C // heads).transpose(1, 2).double()
    p = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) * (C // heads) ** -0.5, dim=-1)
    return (p @ sp(v)).transpose(1, 2).reshape(B, T, C)


def test_cross_attention_with_image_keys_is_the_decoupled_block():
    g = torch.Generator().manual_seed(2)
    a = Attention(64, 48, 16).eval()
    x, ctx = torch.randn(2, 9, 64, generator=g), torch.randn(2, 5, 48, generator=g)
    ip = [(torch.randn(2, 4, 64, generator=g), torch.randn(2, 4, 64, generator=g)) for _ in range(2)]
    scales = torch.tensor([0.6, -0.5])
    a.__dict__["_ip"] = (ip, scales)
    with torch.no_grad():
        got = a(x, ctx)
        q = a.to_q(x)
        want = _attn(q, a.to_k(ctx), a.to_v(ctx), 4) + sum(s * _attn(q, k, v, 4) for s, (k, v) in zip(scales.tolist(), ip))
        torch.testing.assert_close(got, a.to_out[0](want.float()), rtol=1e-4, atol=1e-5)
        assert "_ip" not in a.__dict__                                  # read once
        plain = a(x, ctx)
        a.__dict__["_ip"] = (ip, torch.zeros(2))
        assert torch.equal(a(x, ctx), plain)


def test_unet_forward_with_ip_and_the_refusals():
    from mixdq_amd import Sampler
    unet = build_unet("cpu", dtype=torch.float32, cfg=TINY)
    ad = build_ip_adapter(TINY, 24, dtype=torch.float32)
    g = torch.Generator().manual_seed(3)
    inp = dict(sample=torch.randn(2, 4, 8, 8, generator=g), timestep=torch.tensor(500.0),
               encoder_hidden_states=torch.randn(2, 7, 48, generator=g),
               added_cond_kwargs=dict(text_embeds=torch.randn(2, 40, generator=g), time_ids=torch.rand(2, 6, generator=g)))
    kv = ad.kv(ad.tokens(torch.randn(2, 24, generator=torch.Generator().manual_seed(4))))
    layers = len(ad.dims)
    with torch.no_grad():
        plain = unet(**inp)[0]
        on = unet(**inp, ip=IPState([kv], torch.full((layers, 1), 0.8)))[0]
        only_last = torch.zeros(layers, 1)
        only_last[-1] = 0.8
        assert not torch.equal(on, plain) and not torch.equal(unet(**inp, ip=IPState([kv], only_last))[0], on)
        assert torch.equal(unet(**inp, ip=IPState([kv], torch.zeros(layers, 1)))[0], plain)
        assert torch.equal(unet(**inp)[0], plain)                       # nothing is left behind
        for bad in (IPState([kv[:1]], torch.ones(layers, 1)), IPState([kv], torch.ones(layers + 1, 1)),
                    IPState([kv[..., :-2]], torch.ones(layers, 1)), IPState([kv] * 5, torch.ones(layers, 5)), object()):
            with pytest.raises(RuntimeError):
                unet(**inp, ip=bad)
    with pytest.raises(TypeError):
        Sampler(unet, "euler", 3, 7.5, ip_adapter=object())
    with pytest.raises(ValueError):
        Sampler(unet, "euler", 3, 7.5, ip_adapter=[ad] * 5)
    with pytest.raises(ValueError):
        Sampler(unet, "euler", 3, 7.5, image_guidance_scale=1.5, ip_adapter=ad)
    with pytest.raises(RuntimeError):
        ad.kv(torch.zeros(2, 4, 47))
