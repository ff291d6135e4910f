"""GPU tests of the FP16 VAE decoder (mixdq_amd.vae) on a small config that still reaches every kernel of the full one:
the 4-channel convs on the small-C kernel, 3x3 / 1x1 convs on the MFMA tiles with the residual fold, the upsample
fold, GroupNorm (+SiLU) with FP16 output, the fused q|k|v projection, attention at head width 512 and the padded
conv_out.

Bound: this is a floating-point network with no reference counterpart.  The oracle is the same network built from
stock torch modules (tests/vae_ref.py) in FP32 on the CPU with the same weights upcast; the yardstick for "as good
as FP16 can be" is that stock network run in FP16 on the GPU.  Required: max |decode - fp32| <= 1.5 x max |stock fp16 -
fp32| (the margin of test_norm_mean_over_sigma_envelope), with a floor of one FP16 ulp of the output range.
"""
import pytest
import torch

from tests import vae_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_TINY = 32


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def small():
    from mixdq_amd import vae as V
    cfg = dict(V.VAE_SDXL_CONFIG, block_out_channels=(32, 64, 128, 512), layers_per_block=1, norm_num_groups=8)
    vae = V.build_vae_decoder(cfg, seed=11, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(12)
    latents = (torch.randn(2, 4, 8, 10, generator=g) * cfg["scaling_factor"]).to(DEV)     # as a sampler leaves them
    with torch.no_grad():
        image = vae.decode(latents)
    torch.cuda.synchronize()
    return dict(cfg=cfg, vae=vae, latents=latents, image=image)


def test_vae_decode_vs_the_stock_network(small):
    cfg, vae, latents, image = small["cfg"], small["vae"], small["latents"], small["image"]
    assert image.dtype == torch.float16 and tuple(image.shape) == (2, 3, 64, 80)
    assert bool(torch.isfinite(image).all())
    sd = vae.state_dict()
    ref = vae_ref.stock_decoder(cfg, sd, torch.float32, "cpu")(latents.cpu().float())
    stock16 = vae_ref.stock_decoder(cfg, sd, torch.float16, DEV)(latents).float().cpu()
    err_ours = (image.float().cpu() - ref).abs().max().item()
    err_stock = (stock16 - ref).abs().max().item()
    amax = ref.abs().max().item()
    ulp = 2.0 ** (torch.tensor(amax).log2().floor().item() - 10)          # one FP16 ulp at the top of the output range
    print(f"vae small: max |ref| {amax:.4f}, max err ours {err_ours:.3e}, stock fp16 {err_stock:.3e}, ulp floor {ulp:.3e}")
    assert amax > 1e-2                                                   # (the comparison is of something)
    assert err_ours <= max(1.5 * err_stock, ulp)
    # FP16 latents are taken as they are
    assert torch.equal(bits(vae.decode(latents.half())), bits(vae.decode(latents.half().float())))


def test_vae_graph_replay_equals_eager_bit_for_bit(small):
    from mixdq_amd import vae as V
    from mixdq_amd.quantize_sdxl import hip_graph_opt
    vae = V.build_vae_decoder(small["cfg"], seed=11, device=DEV)
    hip_graph_opt(vae)
    first = vae.decode(small["latents"]).clone()
    assert torch.equal(bits(first), bits(small["image"]))
    other = small["latents"].flip(0).contiguous()
    eager = small["vae"].decode(other)
    assert torch.equal(bits(vae.decode(other)), bits(eager))              # the same graph on other inputs
    assert len(vae.forward._cached) == 1
    assert torch.equal(bits(vae.decode(small["latents"])), bits(small["image"]))


def test_vae_graph_replay_sees_a_later_load_state_dict(small):
    """A captured decode holds the addresses of the parameters AND of the tensors derived from them (q|k|v, the padded
    conv_out, the scaled post_quant_conv) and of the GroupNorm workspaces; load_state_dict rewrites the first two in
    place and keeps the third, so a replay computes with the new weights."""
    from mixdq_amd import vae as V
    from mixdq_amd.quantize_sdxl import hip_graph_opt
    vae = V.build_vae_decoder(small["cfg"], seed=11, device=DEV)
    donor = V.build_vae_decoder(small["cfg"], seed=12, device=DEV)
    want = donor.decode(small["latents"])
    hip_graph_opt(vae)
    before = vae.decode(small["latents"]).clone()
    assert torch.equal(bits(before), bits(small["image"]))
    held = {k: list(v) for k, v in vae._derived().items()}          # (kept alive: their addresses cannot be handed out again)
    ptrs = {k: [t.data_ptr() for t in v] for k, v in held.items()}
    assert set(ptrs) == {"qkv", "conv_out", "post_quant"}
    ws = {k: v.data_ptr() for k, v in vae._gn_ws.items()}
    assert ws
    vae.load_state_dict(donor.state_dict())
    assert {k: [t.data_ptr() for t in v] for k, v in vae._derived().items()} == ptrs
    assert {k: v.data_ptr() for k, v in vae._gn_ws.items()} == ws
    after = vae.decode(small["latents"])
    assert len(vae.forward._cached) == 1                               # a replay, not a new capture
    assert torch.equal(bits(after), bits(want))
    assert not torch.equal(bits(after), bits(before))


def test_vae_batch_row_equals_the_image_alone(small):
    vae = small["vae"]
    for i in range(2):
        alone = vae.decode(small["latents"][i:i + 1])
        assert torch.equal(bits(alone), bits(small["image"][i:i + 1])), i


@pytest.fixture(scope="module")
def tiny_unet(C):
    """The tiny W8A8 UNet of tests/test_sampler_gpu.py (latent 32)."""
    import bench
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet, quantizable_layers
    unet = build_unet(DEV, cfg=dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64))
    inputs = example_inputs(2, L_TINY, DEV, seed=7)
    ckpt = calibrate(unet, [inputs])
    bos_dict = precompute_bos(unet, inputs["encoder_hidden_states"])
    names = list(quantizable_layers(unet))
    quantize_unet(unet, bench.Cfg({n: 8 for n in names}, {n: 8 for n in names if n not in ("conv_in", "conv_out")}),
                  ckpt, bos=True, bos_dict=bos_dict)
    unet.set_fused(True)
    yield unet
    del unet
    torch.cuda.empty_cache()


def test_sampler_sample_image_is_sample_then_decode(small, tiny_unet):
    from mixdq_amd import Sampler
    from mixdq_amd.quantize_sdxl import example_inputs
    vae = small["vae"]
    sm = Sampler(tiny_unet, "euler", 2)
    inp = example_inputs(1, L_TINY, DEV, seed=21)
    noise = torch.randn(1, 4, L_TINY, L_TINY, generator=torch.Generator(device="cpu").manual_seed(22)).to(DEV)
    args = (noise, inp["encoder_hidden_states"], inp["added_cond_kwargs"])
    latents, image = sm.sample_image(vae, *args)
    want = sm.sample(*args)
    assert latents.dtype == torch.float32 and torch.equal(latents, want)
    assert image.dtype == torch.float16 and tuple(image.shape) == (1, 3, 8 * L_TINY, 8 * L_TINY)
    assert torch.equal(bits(image), bits(vae.decode(want)))
