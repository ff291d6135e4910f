"""Host tests of image-to-image in mixdq_amd.sampler (no GPU): the start index against diffusers' get_timesteps, the
start scalars against the schedulers' add_noise / scale_model_input formulas, and the argument checks of
sample(init_latents=...)."""
import numpy as np
import pytest
import torch

from mixdq_amd import sampler as S


def test_img2img_start_table():
    for (n, s), want in {(4, 0.5): 2, (2, 0.5): 1, (1, 1.0): 0, (4, 0.3): 3, (10, 0.7): 3, (10, 0.3): 7,
                         (20, 0.35): 13, (4, 1.0): 0, (50, 0.8): 10}.items():
        assert S.img2img_start(n, s) == want, (n, s)
    with pytest.raises(ValueError, match="no step"):
        S.img2img_start(4, 0.2)
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="strength"):
            S.img2img_start(4, bad)


@pytest.mark.parametrize("kind", S.KINDS)
def test_schedule_start_is_add_noise_and_scale_model_input(kind):
    n = 4
    sch = S.Schedule(kind, n)
    ac = S.alphas_cumprod()
    for t0 in range(n):
        a0, c0, s0 = sch.start(t0)
        assert all(isinstance(v, float) for v in (a0, c0, s0))
        t = int(sch.timesteps[t0])
        if kind == "lcm":
            want = (np.sqrt(ac[t]), np.sqrt(1.0 - ac[t]), 1.0)
        else:
            sigma = np.sqrt((1.0 - ac[t]) / ac[t])
            assert sigma == sch.sigmas[t0]
            want = (1.0, sigma, 1.0 / np.sqrt(sigma ** 2 + 1.0))
        assert (a0, c0, s0) == tuple(float(v) for v in want)
    if kind != "lcm":      # at step 0 the start scalars are the text-to-image ones (euler: init_scale = sigma_0)
        assert sch.start(0)[2] == sch.input_scale0
    if kind == "euler":
        assert sch.start(0)[1] == sch.init_scale
    for bad in (-1, n):
        with pytest.raises(ValueError, match="t0"):
            sch.start(bad)


@pytest.mark.parametrize("n,t0", [(4, 2), (4, 3), (10, 7), (20, 13), (4, 0)])
def test_euler_tail_coefficients_sum_to_minus_sigma(n, t0):
    """x_end = x_t0 + sum_i b_i e_i; with x_t0 = z + sigma_t0 * noise, a UNet that returned the added noise gives z
    back exactly when sum(b[t0:]) == -sigma_t0."""
    sch = S.Schedule("euler", n)
    assert (sch.coef[:, 0] == 1).all() and (sch.coef[:, 2] == 0).all()
    total = sch.coef[t0:, 1].astype(np.float64).sum()
    assert abs(total + sch.sigmas[t0]) <= 1e-6 * sch.sigmas[t0]


def test_sample_checks_its_img2img_arguments():
    """The checks come before anything touches the UNet or the GPU: a Sampler around None is enough."""
    sm = S.Sampler(None, "euler", 4)
    noise = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        sm.sample(noise, None, init_latents=noise, strength=0.5)

    class FakeCuda(torch.Tensor):          # a CPU tensor that says it is on the GPU: reaches the checks behind that one
        is_cuda = True
    fake = torch.zeros(1, 4, 8, 8).as_subclass(FakeCuda)
    with pytest.raises(RuntimeError, match="go together"):
        sm.sample(fake, None, init_latents=noise)
    with pytest.raises(RuntimeError, match="go together"):
        sm.sample(fake, None, strength=0.5)
    with pytest.raises(RuntimeError, match="init_latents should be"):
        sm.sample(fake, None, init_latents=torch.zeros(1, 4, 8, 9), strength=0.5)
    with pytest.raises(RuntimeError, match="init_latents should be"):
        sm.sample(fake, None, init_latents=torch.zeros(1, 4, 8, 8, dtype=torch.float64), strength=0.5)
    with pytest.raises(RuntimeError, match="init_latents should be"):
        sm.sample(fake, None, init_latents=[1.0], strength=0.5)
    with pytest.raises(ValueError, match="no step"):
        sm.sample(fake, None, init_latents=noise, strength=0.2)
    with pytest.raises(ValueError, match="strength"):
        sm.sample(fake, None, init_latents=noise, strength=1.5)
