"""Sampler.inpaint(crop=...) on the GPU: "inpaint only the masked region" on a photograph whose sizes are no multiples
of 8 -- resize the window to the model size, inpaint there, paste the decode back under the (blurred) mask -- against
its seven steps done by hand, bit for bit, on the tiny UNet (latent 32, model 256 px) and the small VAE of
tests/test_inpaint_gpu.py; and that the old paths of the same Sampler do not move."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_TINY = 32
S = 8 * L_TINY
H0, W0 = 360, 400
BOX = (101, 57, 293, 249)


@pytest.fixture(scope="module")
def models(C):
    """(the tiny W8A8 UNet of tests/test_inpaint_gpu.py, a small VAE encoder, its decoder)."""
    import bench
    from mixdq_amd import vae as V
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
    cfg = dict(V.VAE_SDXL_CONFIG, block_out_channels=(32, 64, 128, 512), layers_per_block=1, norm_num_groups=8)
    enc, dec = V.build_vae_encoder(cfg, seed=11, device=DEV), V.build_vae_decoder(cfg, seed=11, device=DEV)
    yield unet, enc, dec
    del unet, enc, dec
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def case():
    from mixdq_amd.quantize_sdxl import example_inputs
    inp = example_inputs(1, L_TINY, DEV, seed=91)
    g = torch.Generator(device="cpu").manual_seed(93)
    noise = torch.randn(1, 4, L_TINY, L_TINY, generator=g).to(DEV)
    photo = torch.randint(0, 256, (1, 3, H0, W0), generator=g, dtype=torch.uint8).to(DEV)
    mask = torch.zeros((1, H0, W0), dtype=torch.uint8, device=DEV)
    mask[:, 100:211, 150:262] = 255                               # inside BOX, edges inside 8x8 blocks of the model grid
    mask[:, 120:130, 160:170] = 0                                 # a hole
    return photo, mask, noise, inp["encoder_hidden_states"], inp["added_cond_kwargs"]


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                      b.contiguous().view(torch.uint8))


def test_cropped_inpaint_is_its_seven_steps(models, case):
    from mixdq_amd import Sampler, _C
    from mixdq_amd import image as I
    unet, enc, dec = models
    photo, mask, noise, ehs, added = case
    sm = Sampler(unet, "euler", 2)
    before = photo.clone()
    latents, image = sm.inpaint(enc, dec, photo, mask, noise, ehs, added, strength=0.5, mask_mode="any", composite=True,
                                crop=BOX)
    assert torch.equal(photo, before)
    # by hand
    small = I.resize(photo, (S, S), BOX, "lanczos3")
    small_mask = I.resize(mask[:, None], (S, S), BOX, "bilinear", mask=True)[:, 0]
    assert small.dtype == torch.uint8 and tuple(small.shape) == (1, 3, S, S) and tuple(small_mask.shape) == (1, S, S)
    m = _C.mask_to_latent(small_mask, "any")
    assert 0 < float(m.sum()) < m.numel()
    want = sm.sample(noise, ehs, added, init_latents=enc.encode(small, None), strength=0.5, mask=m)
    assert latents.dtype == torch.float32 and _bits_equal(latents, want) and bool(torch.isfinite(latents).all())
    pasted = I.paste(dec.decode(want), photo, mask, BOX, "lanczos3")
    assert image.dtype == torch.uint8 and tuple(image.shape) == (1, 3, H0, W0) and torch.equal(image, pasted)
    # every pixel outside the box, and every pixel where the mask is not set, is the input's own byte
    x0, y0, x1, y1 = BOX
    outside = torch.ones_like(image, dtype=torch.bool)
    outside[:, :, y0:y1, x0:x1] = False
    assert torch.equal(image[outside], photo[outside])
    unset = (mask < 128)[:, None].expand_as(image)
    assert torch.equal(image[unset], photo[unset])
    assert not torch.equal(image[~unset], photo[~unset])
    # where it is set: the decode, resized to the window, as pixels
    back = I.resize(dec.decode(want), (y1 - y0, x1 - x0), None, "lanczos3", out="u8_unit")
    win_set = ~unset[:, :, y0:y1, x0:x1]
    assert torch.equal(image[:, :, y0:y1, x0:x1][win_set], back[win_set])
    # the other resampling filters, a [B, 1, H, W] mask and one box per image are the same path
    lat2, img2 = sm.inpaint(enc, dec, photo, mask[:, None], noise, ehs, added, strength=0.5, mask_mode="any",
                            composite=True, crop=[BOX])
    assert _bits_equal(lat2, latents) and torch.equal(img2, image)
    lat3, img3 = sm.inpaint(enc, dec, photo, mask, noise, ehs, added, strength=0.5, mask_mode="any", composite=True,
                            crop=BOX, resample="bicubic")
    assert not torch.equal(img3, image) and torch.equal(img3[outside], photo[outside])


def test_auto_crop_is_the_box_of_bbox_and_crop_region(models, case):
    from mixdq_amd import Sampler
    from mixdq_amd import image as I
    unet, enc, dec = models
    photo, mask, noise, ehs, added = case
    sm = Sampler(unet, "euler", 2)
    bb = I.mask_bbox(mask)
    assert bb == [(150, 100, 262, 211)]
    box = I.crop_region(bb[0], (H0, W0), (S, S), 20)
    assert box == (130, 80, 282, 232)                             # 112x111 grown to 152x151, then 152x152
    auto = sm.inpaint(enc, dec, photo, mask, noise, ehs, added, strength=0.5, composite=True, crop="auto", crop_pad=20)
    explicit = sm.inpaint(enc, dec, photo, mask, noise, ehs, added, strength=0.5, composite=True, crop=box)
    assert _bits_equal(auto[0], explicit[0]) and torch.equal(auto[1], explicit[1])
    outside = torch.ones_like(auto[1], dtype=torch.bool)
    outside[:, :, box[1]:box[3], box[0]:box[2]] = False
    assert torch.equal(auto[1][outside], photo[outside]) and not torch.equal(auto[1], photo)


def test_blurred_mask_feathers_the_paste(models, case):
    from mixdq_amd import Sampler
    from mixdq_amd import image as I
    unet, enc, dec = models
    photo, mask, noise, ehs, added = case
    sm = Sampler(unet, "euler", 2)
    latents, image = sm.inpaint(enc, dec, photo, mask, noise, ehs, added, strength=0.5, composite=True, crop=BOX,
                                mask_blur=3)
    hard_lat, hard = sm.inpaint(enc, dec, photo, mask, noise, ehs, added, strength=0.5, composite=True, crop=BOX)
    assert _bits_equal(latents, hard_lat)                         # the blur touches the paste only
    soft = I.blur_mask(mask, 3)
    assert torch.equal(image, I.paste(dec.decode(latents), photo, soft, BOX, "lanczos3", soft=True))
    zero = (soft == 0)[:, None].expand_as(image)
    assert bool(zero.any()) and torch.equal(image[zero], photo[zero])
    full = (soft == 255)[:, None].expand_as(image)
    assert bool(full.any()) and torch.equal(image[full], hard[full])
    feather = ((soft > 0) & (soft < 255))[:, None].expand_as(image)
    assert bool(feather.any()) and not torch.equal(image[feather], hard[feather])
    x0, y0, x1, y1 = BOX
    outside = torch.ones_like(image, dtype=torch.bool)
    outside[:, :, y0:y1, x0:x1] = False
    assert torch.equal(image[outside], photo[outside])


def test_one_sampler_serves_cropped_plain_and_sample_calls(models, case):
    """crop=None is the old path, and a cropped call between two old ones moves nothing."""
    from mixdq_amd import Sampler
    unet, enc, dec = models
    photo, mask, noise, ehs, added = case
    g = torch.Generator(device="cpu").manual_seed(94)
    pixels = torch.randint(0, 256, (1, 3, S, S), generator=g, dtype=torch.uint8).to(DEV)
    small_mask = torch.zeros((1, S, S), dtype=torch.uint8, device=DEV)
    small_mask[:, 37:150, 60:201] = 255
    sm = Sampler(unet, "euler", 2)
    calls = {"plain": lambda: sm.inpaint(enc, dec, pixels, small_mask, noise, ehs, added, strength=0.5, composite=True),
             "none": lambda: sm.inpaint(enc, dec, pixels, small_mask, noise, ehs, added, strength=0.5, composite=True,
                                        crop=None, crop_pad=7, mask_blur=2.0, resample="bilinear"),
             "f16": lambda: sm.inpaint(enc, dec, pixels, small_mask, noise, ehs, added, strength=0.5),
             "cropped": lambda: sm.inpaint(enc, dec, photo, mask, noise, ehs, added, strength=0.5, composite=True,
                                           crop=BOX),
             "sample": lambda: (sm.sample(noise, ehs, added), None)}
    first = {k: calls[k]() for k in ("plain", "cropped", "sample", "f16")}
    assert first["f16"][1].dtype == torch.float16 and tuple(first["cropped"][1].shape) == (1, 3, H0, W0)
    for k in ("none", "cropped", "plain", "sample", "cropped", "none", "f16"):
        lat, img = calls[k]()
        want = first["plain" if k == "none" else k]
        assert _bits_equal(lat, want[0]), k
        assert img is None or _bits_equal(img, want[1]), k
    # the whole image as the box at the model's own size: bilinear at 1:1 has the weights 1 and 0, so every step is the
    # old path's
    lat, img = sm.inpaint(enc, dec, pixels, small_mask, noise, ehs, added, strength=0.5, composite=True,
                          crop=(0, 0, S, S), resample="bilinear")
    assert _bits_equal(lat, first["plain"][0]) and torch.equal(img, first["plain"][1])
