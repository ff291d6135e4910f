"""Host tests of the VAE encoder in mixdq_amd.vae (no GPU): the parameter inventory against diffusers' AutoencoderKL,
the state dict round trip, the padded conv_in, from_uint8 over all 256 pixel values, and the refusals."""
import numpy as np
import pytest
import torch

from mixdq_amd import derived

from mixdq_amd import vae as V
from tests import vae_enc_ref as ER

SMALL = dict(V.VAE_SDXL_CONFIG, block_out_channels=(32, 64, 128, 512), layers_per_block=1, norm_num_groups=8)


def _expected_names(block_out=(128, 256, 512, 512), layers=2):
    """The issue's name list, expanded by hand: which ResNets carry a conv_shortcut follows from the channel plan."""
    res = ("norm1", "conv1", "norm2", "conv2")
    mods = ["quant_conv", "encoder.conv_in", "encoder.conv_norm_out", "encoder.conv_out"]
    mods += [f"encoder.mid_block.resnets.{j}.{m}" for j in (0, 1) for m in res]
    mods += [f"encoder.mid_block.attentions.0.{m}" for m in ("group_norm", "to_q", "to_k", "to_v", "to_out.0")]
    for i, cout in enumerate(block_out):
        cin = block_out[max(i - 1, 0)]
        for j in range(layers):
            mods += [f"encoder.down_blocks.{i}.resnets.{j}.{m}" for m in res]
            if j == 0 and cin != cout:
                mods.append(f"encoder.down_blocks.{i}.resnets.{j}.conv_shortcut")
        if i != len(block_out) - 1:
            mods.append(f"encoder.down_blocks.{i}.downsamplers.0.conv")
    return {m + s for m in mods for s in (".weight", ".bias")}


@pytest.mark.parametrize("cfg", [V.VAE_SDXL_CONFIG, V.VAE_SD15_CONFIG], ids=["sdxl", "sd15"])
def test_encoder_has_diffusers_parameter_counts_and_names(cfg):
    enc = V.build_vae_encoder(cfg)
    counts = V.parameter_counts(enc)
    assert counts["encoder"] == 34_163_592 and counts["quant_conv"] == 72
    sd = enc.state_dict()
    assert len(sd) == 108
    assert set(sd) == _expected_names() == set(V.encoder_state_dict_names(cfg))
    assert len(V.encoder_state_dict_names(cfg)) == 108
    # with the decoder: the whole AutoencoderKL
    dec = V.parameter_counts(V.build_vae_decoder(cfg))
    assert sum(counts.values()) + sum(dec.values()) == 83_653_863
    assert {n for n in sd if "conv_shortcut.weight" in n} == {
        "encoder.down_blocks.1.resnets.0.conv_shortcut.weight", "encoder.down_blocks.2.resnets.0.conv_shortcut.weight"}
    assert sd["encoder.down_blocks.0.downsamplers.0.conv.weight"].shape == (128, 128, 3, 3)
    assert sd["encoder.conv_in.weight"].shape == (128, 3, 3, 3) and sd["encoder.conv_out.weight"].shape == (8, 512, 3, 3)
    assert sd["quant_conv.weight"].shape == (8, 8, 1, 1)
    assert all(p.dtype == torch.float16 for p in enc.parameters())
    assert enc.scaling_factor == cfg["scaling_factor"]


def test_small_config_names_and_the_stock_network_takes_the_state_dict():
    enc = V.build_vae_encoder(SMALL)
    assert set(enc.state_dict()) == _expected_names((32, 64, 128, 512), 1) == set(V.encoder_state_dict_names(SMALL))
    stock = ER.stock_encoder(SMALL, enc.state_dict(), torch.float32, "cpu")          # strict=True inside
    assert tuple(stock(torch.zeros(1, 3, 16, 24)).shape) == (1, 8, 2, 3)


def test_load_state_dict_round_trips_and_drops_the_derived_weights():
    a, b = V.build_vae_encoder(SMALL, seed=1), V.build_vae_encoder(SMALL, seed=2)
    sd = a.state_dict()
    assert not torch.equal(sd["encoder.conv_in.weight"], b.state_dict()["encoder.conv_in.weight"])
    qkv_before, conv_in_before = b._derived()["qkv"][0].clone(), b._derived()["conv_in"][0].clone()
    ptrs = {k: [t.data_ptr() for t in v] for k, v in b._derived().items()}
    assert set(ptrs) == {"qkv", "conv_in"}
    b._gn_ws["kept"] = ws = object()                 # (the GroupNorm workspaces depend on shapes only: a load keeps them)
    missing, unexpected = b.load_state_dict(sd)
    assert not missing and not unexpected
    # the derived tensors are rewritten at their addresses (a captured graph holds them), not dropped
    assert {k: [t.data_ptr() for t in derived.stored(derived.holder_of(b), k)] for k in derived.holder_of(b)} == ptrs
    assert b._gn_ws == {"kept": ws}
    got = b.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    attn = b.encoder.mid_block.attentions[0]
    w, bias = b._derived()["qkv"]
    assert not torch.equal(w, qkv_before) and not torch.equal(b._derived()["conv_in"][0], conv_in_before)
    assert torch.equal(w, torch.cat([attn.to_q.weight, attn.to_k.weight, attn.to_v.weight])) and w.shape == (1536, 512)
    assert torch.equal(bias, torch.cat([attn.to_q.bias, attn.to_k.bias, attn.to_v.bias]))
    assert torch.equal(b._derived()["conv_in"][0][:, :3], a.encoder.conv_in.weight)
    assert not b._derived()["conv_in"][0][:, 3:].any() and torch.equal(b._derived()["conv_in"][1], a.encoder.conv_in.bias)
    # a move or a dtype change does drop them, and the workspaces; the decoder keeps the same handling from the shared base
    b._derived()
    b.float()
    assert not derived.holder_of(b) and b._gn_ws == {}
    b._derived()
    b.half()
    assert not derived.holder_of(b)
    # load_state_dict(assign=True) puts other tensors in the parameters' place: with another dtype the cache starts over
    b._derived()
    b.load_state_dict({k: v.float() for k, v in sd.items()}, assign=True)
    assert not derived.holder_of(b) and b._derived()["conv_in"][0].dtype == torch.float32
    assert isinstance(b, V._VaeHalf) and isinstance(V.build_vae_decoder(SMALL), V._VaeHalf)


def test_conv_in_is_padded_to_eight_input_channels():
    enc = V.build_vae_encoder(SMALL)
    w8, b8 = enc.padded_conv_in()
    w, b = enc.encoder.conv_in.weight, enc.encoder.conv_in.bias
    assert tuple(w.shape) == (32, 3, 3, 3) and tuple(w8.shape) == (32, 8, 3, 3)
    assert torch.equal(w8[:, :3], w) and not w8[:, 3:].any() and torch.equal(b8, b)
    assert w8.is_contiguous(memory_format=torch.channels_last)
    # the conv of the zero-extended image on the padded weight is the conv (FP32 on the CPU: the op is not at issue)
    x = torch.randn(1, 3, 5, 6, generator=torch.Generator().manual_seed(3))
    x8 = torch.cat([x, torch.zeros(1, 5, 5, 6)], 1)
    assert torch.equal(torch.nn.functional.conv2d(x8, w8.float(), b8.float(), padding=1),
                       torch.nn.functional.conv2d(x, w.float(), b.float(), padding=1))


def test_from_uint8_all_256_values():
    u = torch.arange(256, dtype=torch.uint8)
    got = V.from_uint8(u)
    assert got.dtype == torch.float16
    bits = got.numpy().view(np.uint16)
    # (1) f16(u / 127.5 - 1) computed in float64
    exact = (np.arange(256, dtype=np.float64) / 127.5 - 1.0).astype(np.float16)
    assert np.array_equal(bits, exact.view(np.uint16))
    # (2) diffusers' FP32 order (u / 255) * 2 - 1, rounded to FP16
    f = np.arange(256, dtype=np.float32)
    diff = ((f / np.float32(255.0)) * np.float32(2.0) - np.float32(1.0)).astype(np.float16)
    assert np.array_equal(bits, diff.view(np.uint16))
    # (3) to_uint8 inverts it
    assert torch.equal(V.to_uint8(got), u)
    # ... and it is the ingest kernel's arithmetic as the numpy restatement writes it (constant 0x3C008081)
    assert ER.TWO_OVER_255 == np.float32(2.0 / 255.0)
    want = ER.ingest(np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16))[..., 0].reshape(-1)
    assert np.array_equal(bits, want.view(np.uint16))
    assert got[0] == -1 and got[255] == 1 and V.from_uint8(torch.zeros(2, 3, 4, 4, dtype=torch.uint8)).shape == (2, 3, 4, 4)


def test_latent_restatement_clamps_the_log_variance(oracle):
    """The numpy restatement the GPU test compares against: logvar -31 acts as -30, 21 as 20; no noise: the mode."""
    L = oracle.lib()
    m = np.zeros((1, 1, 4, 8), dtype=np.float16)
    m[0, 0, :, :4] = 0.5
    m[0, 0, :, 4] = [-31, -30, 20, 21]
    n = np.ones((1, 1, 4, 4), dtype=np.float32)
    z = ER.latent_sample(L, m, n, 0.13025)
    assert z.dtype == np.float32 and z[0, 0, 0, 0] == z[0, 0, 1, 0] and z[0, 0, 2, 0] == z[0, 0, 3, 0]
    assert abs(float(z[0, 0, 2, 0]) / ((0.5 + np.exp(10.0)) * 0.13025) - 1) < 1e-6
    assert abs(float(z[0, 0, 0, 1]) / ((0.5 + 1.0) * 0.13025) - 1) < 1e-6
    assert np.array_equal(ER.latent_sample(L, m, None, 0.13025), m[..., :4].astype(np.float32) * np.float32(0.13025))


def test_encode_refuses_what_it_cannot_run():
    enc = V.build_vae_encoder(SMALL)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        enc.encode(torch.zeros(1, 3, 8, 8))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        enc.moments(torch.zeros(1, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        enc.encode("image")
