"""GPU tests of both halves of the FP16 VAE (mixdq_amd.vae) at VAE_SDXL_CONFIG itself: block_out_channels (128, 256, 512,
512), two layers per block, 32 groups -- the widths tests/test_vae_gpu.py and tests/test_vae_enc_gpu.py (32, 64, 128,
512; one layer; 8 groups) do not have: GroupNorm with groups of 4 channels (every 8-channel octet straddles two), the 3x3
convs over K = 9 x 512, the 256 -> 512 and 128 -> 256 shortcut pairs, the second (third) ResNet of each block.  On a
64 x 80 image (8 x 10 latents, 80 tokens in the mid block), batch 2.

Bound: the small-config tests' own.  The oracle is the same network built from stock torch modules (tests/vae_ref.py,
tests/vae_enc_ref.py) in FP32 on the CPU with the same weights upcast; the yardstick is that stock network in FP16 on the
GPU.  Required: max |ours - fp32| <= max(1.5 x max |stock fp16 - fp32|, one FP16 ulp at max |fp32|), the 1.5 being the
margin of test_norm_mean_over_sigma_envelope.  The three figures are printed and recorded in DESIGN.md sections 3.23 and
3.25.
"""
import pytest
import torch

from tests import vae_enc_ref, vae_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1.5


def bits(t):
    return t.contiguous().view(torch.int16)


def _figures(what, ours, stock16, ref):
    err_ours = (ours.float().cpu() - ref).abs().max().item()
    err_stock = (stock16.float().cpu() - ref).abs().max().item()
    amax = ref.abs().max().item()
    ulp = 2.0 ** (torch.tensor(amax).log2().floor().item() - 10)          # one FP16 ulp at the top of the output range
    print(f"{what}: max |ref| {amax:.4f}, max err ours {err_ours:.3e}, stock fp16 {err_stock:.3e}, ulp floor {ulp:.3e}")
    return amax, err_ours, err_stock, ulp


@pytest.fixture(scope="module")
def decoder():
    from mixdq_amd import vae as V
    cfg = dict(V.VAE_SDXL_CONFIG)
    vae = V.build_vae_decoder(cfg, seed=11, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(12)
    latents = (torch.randn(2, 4, 8, 10, generator=g) * cfg["scaling_factor"]).to(DEV)     # as a sampler leaves them
    image = vae.decode(latents)
    torch.cuda.synchronize()
    return dict(cfg=cfg, vae=vae, latents=latents, image=image)


@pytest.fixture(scope="module")
def encoder():
    from mixdq_amd import vae as V
    cfg = dict(V.VAE_SDXL_CONFIG)
    enc = V.build_vae_encoder(cfg, seed=11, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(12)
    image = (torch.rand(2, 3, 64, 80, generator=g) * 2 - 1).to(DEV)                   # uniform in [-1, 1], FP32
    moments = enc.moments(image)
    torch.cuda.synchronize()
    return dict(cfg=cfg, enc=enc, image=image, moments=moments)


def test_the_config_is_sdxls(decoder, encoder):
    for cfg in (decoder["cfg"], encoder["cfg"]):
        assert tuple(cfg["block_out_channels"]) == (128, 256, 512, 512)
        assert (cfg["layers_per_block"], cfg["norm_num_groups"], cfg["latent_channels"]) == (2, 32, 4)
    assert len(decoder["vae"].decoder.up_blocks[0].resnets) == 3 and len(encoder["enc"].encoder.down_blocks[0].resnets) == 2


def test_sdxl_decode_vs_the_stock_network(decoder):
    cfg, vae, latents, image = (decoder[k] for k in ("cfg", "vae", "latents", "image"))
    assert image.dtype == torch.float16 and tuple(image.shape) == (2, 3, 64, 80)
    assert bool(torch.isfinite(image).all())
    sd = vae.state_dict()
    ref = vae_ref.stock_decoder(cfg, sd, torch.float32, "cpu")(latents.cpu().float())
    stock16 = vae_ref.stock_decoder(cfg, sd, torch.float16, DEV)(latents)
    amax, err_ours, err_stock, ulp = _figures("vae decoder, SDXL config", image, stock16, ref)
    assert amax > 1e-2                                                   # (the comparison is of something)
    assert err_ours <= max(MARGIN * err_stock, ulp)


def test_sdxl_decode_batch_row_equals_the_image_alone(decoder):
    for i in range(2):
        alone = decoder["vae"].decode(decoder["latents"][i:i + 1])
        assert torch.equal(bits(alone), bits(decoder["image"][i:i + 1])), i


def test_sdxl_moments_vs_the_stock_network(encoder):
    cfg, enc, image, moments = (encoder[k] for k in ("cfg", "enc", "image", "moments"))
    assert moments.dtype == torch.float16 and tuple(moments.shape) == (2, 8, 8, 10)
    assert bool(torch.isfinite(moments).all())
    sd = enc.state_dict()
    x16 = image.half()                                              # what the ingest feeds conv_in
    ref = vae_enc_ref.stock_encoder(cfg, sd, torch.float32, "cpu")(x16.float().cpu())
    stock16 = vae_enc_ref.stock_encoder(cfg, sd, torch.float16, DEV)(x16)
    amax, err_ours, err_stock, ulp = _figures("vae encoder, SDXL config", moments, stock16, ref)
    assert amax > 1e-2                                                   # (the comparison is of something)
    assert err_ours <= max(MARGIN * err_stock, ulp)


def test_sdxl_moments_batch_row_equals_the_image_alone(encoder):
    for i in range(2):
        alone = encoder["enc"].moments(encoder["image"][i:i + 1])
        assert torch.equal(bits(alone), bits(encoder["moments"][i:i + 1])), i
