"""Host tests of mixdq_amd.vae (no GPU): the decoder's parameter inventory against diffusers' AutoencoderKL, the state
dict round trip, the padded conv_out and to_uint8."""
import torch

from mixdq_amd import derived

from mixdq_amd import vae as V

SMALL = dict(V.VAE_SDXL_CONFIG, block_out_channels=(32, 64, 128, 512), layers_per_block=1, norm_num_groups=8)


def _expected_names(block_out=(128, 256, 512, 512), layers=2):
    """The issue's name list, expanded by hand: which ResNets carry a conv_shortcut follows from the channel plan."""
    res = ("norm1", "conv1", "norm2", "conv2")
    mods = ["post_quant_conv", "decoder.conv_in", "decoder.conv_norm_out", "decoder.conv_out"]
    mods += [f"decoder.mid_block.resnets.{j}.{m}" for j in (0, 1) for m in res]
    mods += [f"decoder.mid_block.attentions.0.{m}" for m in ("group_norm", "to_q", "to_k", "to_v", "to_out.0")]
    rev = block_out[::-1]
    for i in range(len(rev)):
        cin = rev[max(i - 1, 0)]
        for j in range(layers + 1):
            mods += [f"decoder.up_blocks.{i}.resnets.{j}.{m}" for m in res]
            if j == 0 and cin != rev[i]:
                mods.append(f"decoder.up_blocks.{i}.resnets.{j}.conv_shortcut")
        if i != len(rev) - 1:
            mods.append(f"decoder.up_blocks.{i}.upsamplers.0.conv")
    return {m + s for m in mods for s in (".weight", ".bias")}


def test_sdxl_decoder_has_diffusers_parameter_counts_and_names():
    vae = V.build_vae_decoder(V.VAE_SDXL_CONFIG)
    counts = V.parameter_counts(vae)
    assert counts["decoder"] == 49_490_179 and counts["post_quant_conv"] == 20
    names = set(vae.state_dict().keys())
    assert names == _expected_names() == set(V.state_dict_names())
    # the two ResNets whose channel count changes, and only they, have a shortcut conv
    assert {n for n in names if "conv_shortcut.weight" in n} == {
        "decoder.up_blocks.2.resnets.0.conv_shortcut.weight", "decoder.up_blocks.3.resnets.0.conv_shortcut.weight"}
    assert vae.state_dict()["decoder.mid_block.attentions.0.to_q.weight"].shape == (512, 512)
    assert all(p.dtype == torch.float16 for p in vae.parameters())


def test_configs():
    assert V.VAE_SDXL_CONFIG["scaling_factor"] == 0.13025 and V.VAE_SD15_CONFIG["scaling_factor"] == 0.18215
    for k in ("block_out_channels", "layers_per_block", "latent_channels", "norm_num_groups"):
        assert V.VAE_SD15_CONFIG[k] == V.VAE_SDXL_CONFIG[k]
    assert V.VAE_SDXL_CONFIG["block_out_channels"] == (128, 256, 512, 512)
    assert (V.VAE_SDXL_CONFIG["layers_per_block"], V.VAE_SDXL_CONFIG["latent_channels"],
            V.VAE_SDXL_CONFIG["norm_num_groups"]) == (2, 4, 32)
    assert set(V.build_vae_decoder(SMALL).state_dict()) == _expected_names((32, 64, 128, 512), 1) == set(V.state_dict_names(SMALL))


def test_load_state_dict_round_trips_and_drops_the_derived_weights():
    a, b = V.build_vae_decoder(SMALL, seed=1), V.build_vae_decoder(SMALL, seed=2)
    sd = a.state_dict()
    assert not torch.equal(sd["decoder.conv_in.weight"], b.state_dict()["decoder.conv_in.weight"])
    qkv_before = b._derived()["qkv"][0].clone()
    ptrs = {k: [t.data_ptr() for t in v] for k, v in b._derived().items()}
    assert set(ptrs) == {"qkv", "conv_out", "post_quant"}
    b._gn_ws["kept"] = ws = object()                 # (the GroupNorm workspaces depend on shapes only: a load keeps them)
    missing, unexpected = b.load_state_dict(sd)
    assert not missing and not unexpected
    # the derived tensors are rewritten at their addresses (a captured graph holds them), not dropped
    assert {k: [t.data_ptr() for t in derived.stored(derived.holder_of(b), k)] for k in derived.holder_of(b)} == ptrs
    assert b._gn_ws == {"kept": ws}
    got = b.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    attn = b.decoder.mid_block.attentions[0]
    w, bias = b._derived()["qkv"]
    assert not torch.equal(w, qkv_before)
    assert torch.equal(w, torch.cat([attn.to_q.weight, attn.to_k.weight, attn.to_v.weight])) and w.shape == (1536, 512)
    assert torch.equal(bias, torch.cat([attn.to_q.bias, attn.to_k.bias, attn.to_v.bias]))
    # z / scaling_factor is folded into post_quant_conv's 4 x 4 weight, in FP32
    pw, pb = b._derived()["post_quant"]
    assert torch.equal(pw, (b.post_quant_conv.weight.float() / 0.13025).half()) and torch.equal(pb, b.post_quant_conv.bias)
    w4, b4 = b._derived()["conv_out"]
    assert torch.equal(w4[:3], a.decoder.conv_out.weight) and not w4[3].any()
    assert torch.equal(b4[:3], a.decoder.conv_out.bias) and not b4[3].any()
    # a second load (back to b's first weights) is seen too: nothing was left aliasing a temporary
    b.load_state_dict(V.build_vae_decoder(SMALL, seed=2).state_dict())
    assert torch.equal(b._derived()["qkv"][0], qkv_before) and b._derived()["qkv"][0].data_ptr() == ptrs["qkv"][0]
    # load_state_dict(assign=True) puts other tensors in the parameters' place: with another dtype the cache starts over
    b.load_state_dict({k: v.float() for k, v in sd.items()}, assign=True)
    assert not derived.holder_of(b) and b._gn_ws == {} and b._derived()["qkv"][0].dtype == torch.float32
    # a move or a dtype change drops the derived tensors and the workspaces
    b._gn_ws["dropped"] = object()
    b.half()
    assert not derived.holder_of(b) and b._gn_ws == {}
    b._derived()
    b.to("cpu", torch.float32)
    assert not derived.holder_of(b)


def test_conv_out_is_padded_to_four_channels_and_sliced_back():
    vae = V.build_vae_decoder(SMALL)
    w4, b4 = vae.padded_conv_out()
    w, b = vae.decoder.conv_out.weight, vae.decoder.conv_out.bias
    assert tuple(w.shape) == (3, 32, 3, 3) and tuple(w4.shape) == (4, 32, 3, 3) and tuple(b4.shape) == (4,)
    assert torch.equal(w4[:3], w) and torch.equal(b4[:3], b)
    assert not w4[3].any() and not b4[3].any()
    assert w4.is_contiguous(memory_format=torch.channels_last)
    # the conv on the padded weight, cut to three channels, is the conv (FP32 on the CPU: the op itself is not at issue)
    x = torch.randn(1, 32, 5, 6, generator=torch.Generator().manual_seed(3))
    full = torch.nn.functional.conv2d(x, w4.float(), b4.float(), padding=1)
    assert torch.equal(full[:, :3], torch.nn.functional.conv2d(x, w.float(), b.float(), padding=1))
    assert not full[:, 3].any()


def test_to_uint8_known_values():
    x = torch.tensor([-3.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0, 1.0 / 255, -1.0 + 4.0 / 255])
    assert V.to_uint8(x).tolist() == [0, 0, 64, 128, 191, 255, 255, 128, 2]
    assert V.to_uint8(x.half()).dtype == torch.uint8 and V.to_uint8(torch.zeros(2, 3, 4, 4)).shape == (2, 3, 4, 4)


def test_decode_refuses_what_it_cannot_run():
    import pytest
    vae = V.build_vae_decoder(SMALL)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        vae.decode(torch.zeros(1, 4, 8, 8))


def test_the_conv_launch_enumeration_covers_the_networks_geometries():
    """The list is derived; this names what it must contain (and that the modules built from the same config hold
    exactly these weight shapes, so that a layer added to the network without the walk above shows)."""
    from tests.vae_layers import LAUNCHES
    got = set(LAUNCHES)
    for cin, cout in ((128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (512, 256), (256, 128)):
        assert (cin, cout, 3, 1, None, False) in got, (cin, cout)
    for c in (128, 256, 512):
        assert (c, c, 3, 1, None, True) in got and (c, c, 3, 2, "pad_after", False) in got, c
    assert {g[:2] for g in got if g[2] == 1 and g[0] > 8} == {(128, 256), (256, 512), (512, 256), (256, 128)}
    assert {g[0] for g in got if g[4] == "upsample2x"} == {512, 256}
    assert {(8, 128, 3, 1, None, False), (128, 4, 3, 1, None, False), (512, 8, 3, 1, None, False),
            (8, 8, 1, 1, None, False), (4, 4, 1, 1, None, False), (4, 512, 3, 1, None, False)} <= got
    assert all(residual is False or (cin == cout and k == 3 and flag is None) for cin, cout, k, _, flag, residual in got)
    assert len(LAUNCHES) == len(got) == 25
    # the weight shapes of the two modules, with the derived ones in place of the weights they stand for
    dec, enc = V.build_vae_decoder(V.VAE_SDXL_CONFIG), V.build_vae_encoder(V.VAE_SDXL_CONFIG)
    shapes = {tuple(p.shape) for m in (dec, enc) for n, p in m.named_parameters() if p.dim() == 4}
    shapes -= {tuple(dec.decoder.conv_out.weight.shape), tuple(enc.encoder.conv_in.weight.shape)}
    shapes |= {tuple(dec.padded_conv_out()[0].shape), tuple(enc.padded_conv_in()[0].shape)}
    assert shapes == {(cout, cin, k, k) for cin, cout, k, _, _, _ in got}
