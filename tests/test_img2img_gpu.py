"""Image-to-image on the GPU: Sampler.sample(init_latents=z, strength=s) starts the device-side loop at step t0 =
img2img_start(n_steps, s) and must equal, bit for bit, an eager loop that builds the start state with three torch
operations (two products, one sum), then calls the UNet and the numpy restatement of the step (tests/sampler_ref.py)
for steps t0 .. n - 1; one Sampler serves text-to-image and image-to-image calls alike on one captured graph; and
Sampler.img2img is encode, sample, decode."""
import numpy as np
import pytest
import torch

from tests import sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_TINY = 32


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return a.contiguous().view({2: torch.int16, 4: torch.int32}[a.element_size()])


@pytest.fixture(scope="module")
def tiny_unet(C):
    """The tiny W8A8 UNet of tests/test_vae_gpu.py (latent 32)."""
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


def _inputs(B, rows, seed, n_steps, uses_noise):
    from mixdq_amd.quantize_sdxl import example_inputs
    inp = example_inputs(B * rows, L_TINY, DEV, seed=seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    noise = torch.randn(B, 4, L_TINY, L_TINY, generator=g).to(DEV)
    z = (torch.randn(B, 4, L_TINY, L_TINY, generator=g) * 0.13025).to(DEV)        # as VAEEncoder.encode leaves them
    step_noise = torch.randn(n_steps, B, 4, L_TINY, L_TINY, generator=g).to(DEV) if uses_noise else None
    return z, noise, inp["encoder_hidden_states"], inp["added_cond_kwargs"], step_noise


def _eager_img2img(unet, sampler, z, noise, ehs, added, step_noise, strength):
    from mixdq_amd.sampler import img2img_start
    s, rows = sampler.schedule, sampler.rows_per_image
    B = noise.shape[0]
    t0 = img2img_start(s.n_steps, strength)
    a0, c0, s0 = (torch.tensor(v, dtype=torch.float32, device=DEV) for v in s.start(t0))
    az = z.float() * a0                                  # three torch operations, each rounded to FP32
    cn = noise.float() * c0
    x = az + cn
    inp = (x * s0).to(torch.float16).cpu().numpy()
    x = x.cpu().numpy()
    for i in range(t0, s.n_steps):
        sample = t(np.concatenate([inp] * rows, axis=0))
        with torch.no_grad():
            eps = unet(sample, torch.tensor(float(s.timesteps[i]), device=DEV), ehs, added)[0]
        eps = eps.float().cpu().numpy().astype(np.float16)
        x, inp = R.step(x, eps[:B], eps[B:] if rows == 2 else None, s.coef[i], sampler.guidance_scale,
                        step_noise[i].float().cpu().numpy() if s.uses_noise else None)
    return t0, torch.from_numpy(x)


@pytest.mark.parametrize("kind,n_steps,strength,g", [("euler", 4, 0.5, 0.0), ("euler", 4, 0.5, 5.0),
                                                     ("euler_ancestral", 2, 0.5, 0.0), ("lcm", 4, 0.5, 0.0)])
def test_img2img_sample_equals_the_eager_loop(tiny_unet, kind, n_steps, strength, g):
    from mixdq_amd import Sampler
    sm = Sampler(tiny_unet, kind, n_steps, guidance_scale=g)
    rows = sm.rows_per_image
    assert rows == (2 if g > 1 else 1)
    for seed in (41, 42):                                   # the second run: other inputs, the same graph
        z, noise, ehs, added, sn = _inputs(2, rows, seed, n_steps, sm.schedule.uses_noise)
        graph = sm._graph
        got = sm.sample(noise, ehs, added, sn, init_latents=z, strength=strength)
        assert graph is None or sm._graph is graph
        t0, want = _eager_img2img(tiny_unet, sm, z, noise, ehs, added, sn, strength)
        assert 0 < t0 < n_steps and int(sm._step.item()) == n_steps
        assert got.dtype == torch.float32 and got.shape == noise.shape and bool(torch.isfinite(got).all())
        assert torch.equal(bits(got.cpu()), bits(want)), f"{kind} x {n_steps} from step {t0}, seed {seed}"
    # FP16 latents are taken as they are
    assert torch.equal(bits(sm.sample(noise, ehs, added, sn, init_latents=z.half(), strength=strength)),
                       bits(sm.sample(noise, ehs, added, sn, init_latents=z.half().float(), strength=strength)))
    # strength 1.0 is the whole schedule from a0 * z + c0 * noise
    full = sm.sample(noise, ehs, added, sn, init_latents=z, strength=1.0)
    t0, want = _eager_img2img(tiny_unet, sm, z, noise, ehs, added, sn, 1.0)
    assert t0 == 0 and torch.equal(bits(full.cpu()), bits(want))


def test_one_sampler_serves_text_to_image_and_img2img(tiny_unet):
    from mixdq_amd import Sampler
    sm = Sampler(tiny_unet, "euler_ancestral", 4)
    z, noise, ehs, added, sn = _inputs(1, 1, 51, 4, True)
    first = sm.sample(noise, ehs, added, sn)
    graph = sm._graph
    mid = sm.sample(noise, ehs, added, sn, init_latents=z, strength=0.5)
    third = sm.sample(noise, ehs, added, sn)
    assert sm._graph is graph
    assert torch.equal(bits(first), bits(third)) and not torch.equal(bits(first), bits(mid))
    # ... and the other way round: a Sampler whose graph an img2img call captured
    sm2 = Sampler(tiny_unet, "euler_ancestral", 4)
    assert torch.equal(bits(sm2.sample(noise, ehs, added, sn, init_latents=z, strength=0.5)), bits(mid))
    assert torch.equal(bits(sm2.sample(noise, ehs, added, sn)), bits(first))
    with pytest.raises(RuntimeError, match="go together"):
        sm.sample(noise, ehs, added, sn, init_latents=z)
    with pytest.raises(RuntimeError, match="init_latents should be"):
        sm.sample(noise, ehs, added, sn, init_latents=z[:, :2], strength=0.5)
    with pytest.raises(RuntimeError, match="init_latents should be"):
        sm.sample(noise, ehs, added, sn, init_latents=z.cpu(), strength=0.5)
    assert torch.equal(bits(sm.sample(noise, ehs, added, sn)), bits(first))                  # refusals left it usable


def test_img2img_is_encode_sample_decode(tiny_unet):
    from mixdq_amd import Sampler
    from mixdq_amd import vae as V
    cfg = dict(V.VAE_SDXL_CONFIG, block_out_channels=(32, 64, 128, 512), layers_per_block=1, norm_num_groups=8)
    enc, dec = V.build_vae_encoder(cfg, seed=11, device=DEV), V.build_vae_decoder(cfg, seed=11, device=DEV)
    sm = Sampler(tiny_unet, "euler", 2)
    z, noise, ehs, added, _ = _inputs(1, 1, 61, 2, False)
    g = torch.Generator(device="cpu").manual_seed(62)
    pixels = torch.randint(0, 256, (1, 3, 8 * L_TINY, 8 * L_TINY), generator=g, dtype=torch.uint8).to(DEV)
    latent_noise = torch.randn(1, 4, L_TINY, L_TINY, generator=g).to(DEV)
    for ln in (None, latent_noise):
        latents, image = sm.img2img(enc, dec, pixels, noise, ehs, added, strength=0.5, latent_noise=ln)
        want = sm.sample(noise, ehs, added, init_latents=enc.encode(pixels, ln), strength=0.5)
        assert latents.dtype == torch.float32 and torch.equal(bits(latents), bits(want))
        assert image.dtype == torch.float16 and tuple(image.shape) == (1, 3, 8 * L_TINY, 8 * L_TINY)
        assert torch.equal(bits(image), bits(dec.decode(want)))
