"""The sampler on the GPU: mixdq_sampler_step against its numpy float32 restatement (tests/sampler_ref.py) bit for
bit -- the FP32 state and every written FP16 input row -- its device-side step state, and mixdq_amd.Sampler (one
captured step graph replayed n_steps times) against an eager Python loop that calls the UNet and then the
restatement: bit-equal on the tiny UNet of the glue tests, and once each at full size (SDXL at 1024 px, SD 1.5 at
512 px)."""
import numpy as np
import pytest
import torch

from tests import sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("euler_ancestral", "euler", "lcm")
L_TINY = 32


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.detach().cpu().contiguous().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {g.size} elements differ"


def _up(v, m):
    return (v + m - 1) // m * m


def _run_kernel_steps(C, coef, t_table, n, rows, with_noise, g, seed, start=0, edge=None):
    """Launch the kernel for every step from `start` on freshly drawn eps, checking each launch against the
    restatement.  Row blocks and noise blocks sit at padded strides; the padding must stay untouched."""
    rng = np.random.default_rng(seed)
    n_steps = coef.shape[0]
    rs, ns = _up(n, 8) + 8, _up(n, 4) + 4
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    noise = rng.standard_normal((n_steps, ns)).astype(np.float32) if with_noise else None
    if edge is not None:
        x[:len(edge)] = edge
    x_d = t(x)
    noise_d = t(noise) if with_noise else None
    coef_d, tt_d = t(coef), t(t_table)
    step_d = torch.tensor([start], dtype=torch.int32, device=DEV)
    t_d = torch.tensor(-1.0, dtype=torch.float32, device=DEV)
    pad = np.float16(-7.25)
    for i in range(start, n_steps):
        eps = rng.standard_normal((rows, rs)).astype(np.float16)
        if edge is not None:                    # eps and noise 0 there: the state passes through a * x
            eps[:, :len(edge)] = 0
            if with_noise:
                noise[i, :len(edge)] = 0
                noise_d = t(noise)
        inp_d = torch.full((rows, rs), float(pad), dtype=torch.float16, device=DEV)
        C.sampler_step(x_d, t(eps), inp_d, coef_d, tt_d, step_d, t_d, g, rows, noise_d, n=n, row_stride=rs,
                       noise_stride=ns)
        x, want_in = R.step(x, eps[0, :n], eps[1, :n] if rows == 2 else None, coef[i], g,
                            noise[i, :n] if with_noise else None)
        _same(x_d, x, f"state after step {i}")
        got_in = inp_d.cpu().numpy()
        for r in range(rows):
            _same(got_in[r, :n], want_in, f"UNet input row block {r} after step {i}")
        assert (got_in[:, n:] == pad).all(), "the kernel wrote behind its n elements"
        assert int(step_d.item()) == i + 1 and float(t_d.item()) == float(t_table[i + 1])
    return x, want_in


@pytest.mark.parametrize("n", [8 * 1031, 8 * 1031 + 3, 5], ids=["n8k", "n8k+3", "n5"])
@pytest.mark.parametrize("with_noise", [False, True], ids=["nonoise", "noise"])
@pytest.mark.parametrize("rows", [1, 2], ids=["rows1", "rows2"])
@pytest.mark.parametrize("kind", KINDS)
def test_step_kernel_equals_the_restatement(C, kind, rows, with_noise, n):
    from mixdq_amd.sampler import schedule
    s = schedule(kind, 4)
    for g in (7.5, 0.0) if rows == 2 else (0.0,):
        _run_kernel_steps(C, s.coef, s.t_table, n, rows, with_noise, g,
                          seed=1000 * KINDS.index(kind) + 100 * rows + 10 * with_noise + n % 7)


def test_step_kernel_grid_stride_and_twenty_steps(C):
    """More vectors than the launch has lanes (the grid is capped at 2048 workgroups), and a 20-step table."""
    from mixdq_amd.sampler import schedule
    s = schedule("euler", 20)
    n = 8 * (2048 * 256 + 37) + 5
    _run_kernel_steps(C, s.coef, s.t_table, n, 2, False, 5.0, seed=3, start=18)
    s = schedule("euler_ancestral", 20)
    _run_kernel_steps(C, s.coef, s.t_table, 8 * 515 + 1, 1, True, 0.0, seed=4)


@pytest.mark.parametrize("rows", [1, 2])
def test_step_kernel_fp16_ties_and_overflow(C, rows):
    """With a = 1, s_next = 1 and eps = noise = 0 the next input is f16_rn(x): halfway cases round to even, 65520
    (halfway between the largest finite FP16 and 2^16) and everything above overflow to infinity, values just below
    do not; tiny values reach FP16's subnormals; -0 leaves the sum (-0 + -0) + +0 as +0.  With s_next = 1 + 2^-12 the
    FP32 product is rounded first."""
    h = 2.0 ** -11
    edge = np.array([1 + h, 1 + 3 * h, 1 + 5 * h, -(1 + h), -(1 + 3 * h), 2048 + 1, 2048 + 3, 65520.0, -65520.0,
                     65519.996, 65504.0, 70000.0, -1e9, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24 + 2.0 ** -26, -0.0,
                     1 + h - 2.0 ** -23, 1 + h + 2.0 ** -23], dtype=np.float32)
    for s_next in (1.0, 1.0 + 2.0 ** -12):
        coef = np.array([[1.0, -0.75, 0.5, s_next]], dtype=np.float32)
        _, got = _run_kernel_steps(C, coef, np.array([999.0, 0.0], dtype=np.float32), 8 * 9 + 3, rows, True, 2.0,
                                   seed=11, edge=edge)
        if s_next == 1.0:
            want = np.array([1.0, 1 + 4 * h, 1 + 4 * h, -1.0, -(1 + 4 * h), 2048, 2052, np.inf, -np.inf, 65504, 65504,
                             np.inf, -np.inf, 0.0, 2.0 ** -23, 2.0 ** -24, 0.0, 1.0, 1 + 2 * h], dtype=np.float16)
            _same(got[:len(edge)], want, "FP16 rounding of the edge values")


def test_device_step_state(C):
    """After n launches the timestep tensor holds t_table[n] and the index n; a launch past the table changes
    nothing (state, input, index, timestep)."""
    from mixdq_amd.sampler import schedule
    s = schedule("lcm", 4)
    n = 64
    x_d = t(np.arange(n, dtype=np.float32))
    eps_d = t(np.ones(n, dtype=np.float16))
    inp_d = torch.zeros(n, dtype=torch.float16, device=DEV)
    step_d = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_d = torch.tensor(float(s.t_table[0]), device=DEV)
    coef_d, tt_d = t(s.coef), t(s.t_table)
    for i in range(4):
        assert float(t_d.item()) == float(s.timesteps[i]) and int(step_d.item()) == i
        C.sampler_step(x_d, eps_d, inp_d, coef_d, tt_d, step_d, t_d)
    assert int(step_d.item()) == 4 and float(t_d.item()) == float(s.t_table[4])
    before = (x_d.clone(), inp_d.clone())
    C.sampler_step(x_d, eps_d, inp_d, coef_d, tt_d, step_d, t_d)
    assert int(step_d.item()) == 4 and float(t_d.item()) == float(s.t_table[4])
    assert torch.equal(x_d, before[0]) and torch.equal(inp_d, before[1])
    with pytest.raises(RuntimeError, match="invalid argument"):
        C.sampler_step(x_d, eps_d, inp_d, coef_d, tt_d, step_d, t_d, 0.0, 3)
    with pytest.raises(RuntimeError, match="alignment"):
        C.sampler_step(x_d[1:], eps_d, inp_d, coef_d, tt_d, step_d, t_d, n=32)


# ---- Sampler == the eager loop ---------------------------------------------------------------------------------
def _eager_loop(unet, sampler, noise, ehs, added, step_noise):
    """The loop a user writes around unet(...): NCHW tensors, a host-side timestep, the restatement on the host."""
    s, rows = sampler.schedule, sampler.rows_per_image
    B = noise.shape[0]
    x, inp = R.init(noise.float().cpu().numpy(), s.init_scale, s.input_scale0)
    for i in range(s.n_steps):
        sample = t(np.concatenate([inp] * rows, axis=0))
        with torch.no_grad():
            eps = unet(sample, torch.tensor(float(s.timesteps[i]), device=DEV), ehs, added)[0]
        eps = eps.float().cpu().numpy().astype(np.float16)
        x, inp = R.step(x, eps[:B], eps[B:] if rows == 2 else None, s.coef[i], sampler.guidance_scale,
                        step_noise[i].float().cpu().numpy() if s.uses_noise else None)
    return x


def _inputs(B, rows, L, seed, n_steps, cfg=None, uses_noise=True):
    from mixdq_amd.quantize_sdxl import example_inputs
    inp = example_inputs(B * rows, L, DEV, seed=seed, cfg=cfg)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    noise = torch.randn(B, 4, L, L, generator=g).to(DEV)
    step_noise = torch.randn(n_steps, B, 4, L, L, generator=g).to(DEV) if uses_noise else None
    return noise, inp["encoder_hidden_states"], inp["added_cond_kwargs"], step_noise


def _rows(v, idx):
    if v is None:
        return None
    if isinstance(v, dict):
        return {k: _rows(a, idx) for k, a in v.items()}
    return v[idx].contiguous()


@pytest.fixture(scope="module")
def tiny(C):
    """The tiny UNet of tests/test_glue_gpu.py in its 64-wide-heads form (every attention on this project's
    kernels), latent 32: uniform W8A8 + BOS, the fused graph on."""
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


@pytest.mark.parametrize("kind,n_steps,g", [("euler_ancestral", 1, 0.0), ("euler_ancestral", 4, 0.0), ("lcm", 4, 0.0),
                                            ("euler", 3, 7.5)])
def test_sampler_equals_the_eager_loop_on_the_tiny_unet(tiny, kind, n_steps, g):
    from mixdq_amd import Sampler
    sm = Sampler(tiny, kind, n_steps, guidance_scale=g)
    rows = sm.rows_per_image
    assert rows == (2 if g > 1 else 1)
    for seed in (21, 22):                                   # the second run: other inputs, the same graph
        noise, ehs, added, sn = _inputs(2, rows, L_TINY, seed, n_steps, uses_noise=sm.schedule.uses_noise)
        graph = sm._graph
        got = sm.sample(noise, ehs, added, sn)
        assert graph is None or sm._graph is graph
        assert int(sm._step.item()) == n_steps              # ... and sample() reset the index it had left at n_steps
        assert got.dtype == torch.float32 and got.shape == noise.shape and torch.isfinite(got).all()
        _same(got, _eager_loop(tiny, sm, noise, ehs, added, sn), f"{kind} x {n_steps}, seed {seed}")
    # row i of the batch-2 run == the batch-1 run of that image
    sm1 = Sampler(tiny, kind, n_steps, guidance_scale=g)
    for i in range(2):
        idx = [i] if rows == 1 else [i, 2 + i]
        one = sm1.sample(noise[i:i + 1], _rows(ehs, idx), _rows(added, idx), None if sn is None else sn[:, i:i + 1])
        _same(one, got[i:i + 1], f"row {i} of the batch-2 run != its batch-1 run")
    with pytest.raises(RuntimeError, match="shape"):
        sm1.sample(noise, ehs, added, sn)


def test_sampler_refuses_what_it_cannot_run(tiny):
    from mixdq_amd import Sampler
    noise, ehs, added, sn = _inputs(1, 1, L_TINY, 5, 4)
    with pytest.raises(RuntimeError, match="step_noise"):
        Sampler(tiny, "euler_ancestral", 4).sample(noise, ehs, added)
    with pytest.raises(RuntimeError, match="step_noise"):
        Sampler(tiny, "euler", 4).sample(noise, ehs, added, sn)
    with pytest.raises(RuntimeError, match="rows"):
        Sampler(tiny, "euler", 4, guidance_scale=7.5).sample(noise, ehs, added)


class _Cfg:
    def __init__(self, w, a):
        self.w_config, self.a_config = w, a


def test_full_sdxl_1024px_four_euler_ancestral_steps(C):
    """SDXL at 1024 px (latent 128), uniform W8A8 + BOS, the fused graph: 4 euler_ancestral steps at batch 1."""
    from mixdq_amd import Sampler, cfgs
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet
    unet = build_unet(DEV)
    inputs2 = example_inputs(2, 128, DEV, seed=7)
    ckpt = calibrate(unet, [inputs2])
    quantize_unet(unet, _Cfg(cfgs.load("weight/uniform_8"), cfgs.load("act/act_8.00")), ckpt, bos=True,
                  bos_dict=precompute_bos(unet, inputs2["encoder_hidden_states"]))
    del ckpt
    unet.set_fused(True)
    sm = Sampler(unet, "euler_ancestral", 4)
    noise, ehs, added, sn = _inputs(1, 1, 128, 31, 4)
    got = sm.sample(noise, ehs, added, sn)
    assert torch.isfinite(got).all()
    _same(got, _eager_loop(unet, sm, noise, ehs, added, sn), "SDXL 1024 px, 4 euler_ancestral steps")
    del unet, sm
    torch.cuda.empty_cache()


def test_full_sd15_512px_four_lcm_steps(C):
    """The SD 1.5 UNet at 512 px (latent 64), uniform W8A8 + BOS, the fused graph: 4 lcm steps at batch 1."""
    from mixdq_amd import Sampler
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import SD15_CONFIG, build_unet, quantizable_layers
    unet = build_unet(DEV, cfg=SD15_CONFIG)
    inputs2 = example_inputs(2, 64, DEV, seed=7, cfg=SD15_CONFIG)
    ckpt = calibrate(unet, [inputs2])
    names = list(quantizable_layers(unet))
    quantize_unet(unet, _Cfg({n: 8 for n in names}, {n: 8 for n in names if n not in ("conv_in", "conv_out")}), ckpt,
                  bos=True, bos_dict=precompute_bos(unet, inputs2["encoder_hidden_states"]))
    del ckpt
    unet.set_fused(True)
    sm = Sampler(unet, "lcm", 4)
    noise, ehs, added, sn = _inputs(1, 1, 64, 33, 4, cfg=SD15_CONFIG)
    assert added is None
    got = sm.sample(noise, ehs, added, sn)
    assert torch.isfinite(got).all()
    _same(got, _eager_loop(unet, sm, noise, ehs, added, sn), "SD 1.5 512 px, 4 lcm steps")
    del unet, sm
    torch.cuda.empty_cache()
