"""The multistep sampler on the GPU.  mixdq_sampler_step_2m and mixdq_sampler_step_2m_masked against the numpy
restatement (tests/multistep_ref.py; the blend: tests/inpaint_ref.py) bit for bit -- the FP32 state, the history, every
written FP16 input row, the device step state -- from a history buffer full of NaN, from step 0 and from a later first
step; and Sampler('dpmpp_2m') / Sampler('ddim') (captured step graphs replayed) against an eager loop of UNet calls and
the restatement, bit for bit on the tiny UNet of the sampler tests: text-to-image, image-to-image, inpainting, and all
three in turn on one Sampler."""
import numpy as np
import pytest
import torch

from tests import inpaint_ref as I
from tests import multistep_ref as M
from tests import sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_TINY = 32
f32 = np.float32


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


# ---- the step kernels ----------------------------------------------------------------------------------------------
def _run_2m_steps(C, s, n, rows, g, seed, first=0, start=None, channels=None, mask_kind=None):
    """Launch the step for every step from `start` (default: `first`) of a run whose first step is `first`, on freshly
    drawn eps, and check each launch against the restatement: the state, the history (== this step's x0), every
    written FP16 input row, the padding behind the n elements of the row blocks and of the history, the step index
    and the timestep.  When the first launch is the run's first step the history starts FULL OF NaN: a first-order
    step must not read it.  channels / mask_kind ('zeros', 'ones', 'soft'): the masked form, with the plain form
    launched beside it from the same state -- its history must be the same bits, and with a mask of ones its state
    and input too."""
    rng = np.random.default_rng(seed)
    coef, t_table, blend = s.coef, s.t_table, s.blend
    n_steps = coef.shape[0]
    start = first if start is None else start
    rs, hs = _up(n, 8) + 8, _up(n, 4) + 4
    x = (rng.standard_normal(n) * 1.5).astype(f32)
    hist = np.full(hs, np.nan, dtype=f32)
    if start > first:                                  # mid-run: the previous step left a prediction there
        hist[:n] = rng.standard_normal(n).astype(f32)
    masked = channels is not None
    if masked:
        z = (rng.standard_normal(n) * 0.2).astype(f32)
        n0 = rng.standard_normal(n).astype(f32)
        mask = {"zeros": np.zeros, "ones": np.ones, "soft": lambda k, dtype: rng.random(k).astype(dtype)}[mask_kind](
            n // channels, dtype=f32)
        m_el = np.repeat(mask, channels)
        z_d, n0_d, mask_d, blend_d = t(z), t(n0), t(mask), t(blend)
    x_d, hist_d = t(x), t(hist)
    coef_d, tt_d = t(coef), t(t_table)
    step_d = torch.tensor([start], dtype=torch.int32, device=DEV)
    first_d = torch.tensor([first], dtype=torch.int32, device=DEV)
    t_d = torch.tensor(-1.0, dtype=torch.float32, device=DEV)
    pad = np.float16(-7.25)
    orders = []
    for i in range(start, n_steps):
        eps = rng.standard_normal((rows, rs)).astype(np.float16)
        eps_d = t(eps)
        inp_d = torch.full((rows, rs), float(pad), dtype=torch.float16, device=DEV)
        second = M.is_second(coef[i], i, first)
        orders.append(second)
        y, p = M.step(x, hist[:n], eps[0, :n], eps[1, :n] if rows == 2 else None, coef[i], g, second)
        if masked:
            px_d, ph_d, pstep_d, pt_d = x_d.clone(), hist_d.clone(), step_d.clone(), t_d.clone()
            pin_d = torch.zeros((rows, rs), dtype=torch.float16, device=DEV)
            C.sampler_step_2m(px_d, eps_d, pin_d, ph_d, coef_d, tt_d, pstep_d, first_d, pt_d, g, rows, n=n, row_stride=rs)
            C.sampler_step_2m_masked(x_d, eps_d, inp_d, hist_d, coef_d, tt_d, step_d, first_d, t_d, z_d, n0_d, mask_d,
                                     blend_d, g, rows, channels=channels, n=n, row_stride=rs)
            _same(px_d, y, f"plain state after step {i}")
            _same(ph_d, hist_d, f"masked history != plain history after step {i}")
            x = I.blend(y, z, n0, m_el, blend[i, 0], blend[i, 1])
            if mask_kind == "ones":
                _same(x_d, px_d, f"mask of ones: state != the plain form's after step {i}")
                _same(inp_d[:, :n], pin_d[:, :n], f"mask of ones: input != the plain form's after step {i}")
            if mask_kind == "zeros":
                assert np.array_equal(x_d.cpu().numpy(), I.kept(z, n0, blend[i, 0], blend[i, 1]))
        else:
            C.sampler_step_2m(x_d, eps_d, inp_d, hist_d, coef_d, tt_d, step_d, first_d, t_d, g, rows, n=n, row_stride=rs)
            x = y
        hist[:n] = p
        want_in = M.scaled_input(x, coef[i, 6])
        assert np.isfinite(x).all() and np.isfinite(p).all() and np.isfinite(want_in).all()   # NaN-free: hist not read
        _same(x_d, x, f"state after step {i}")
        got_h = hist_d.cpu().numpy()
        _same(got_h[:n], p, f"history after step {i} (should be this step's x0)")
        assert np.isnan(got_h[n:]).all(), "the kernel wrote behind the history's n elements"
        got_in = inp_d.cpu().numpy()
        for r in range(rows):
            _same(got_in[r, :n], want_in, f"UNet input row block {r} after step {i}")
        assert (got_in[:, n:] == pad).all(), "the kernel wrote behind its n elements"
        assert int(step_d.item()) == i + 1 and float(t_d.item()) == float(t_table[i + 1])
    # one launch past the table changes nothing, the history included
    before = (x_d.clone(), inp_d.clone(), hist_d.clone())
    if masked:
        C.sampler_step_2m_masked(x_d, eps_d, inp_d, hist_d, coef_d, tt_d, step_d, first_d, t_d, z_d, n0_d, mask_d, blend_d,
                                 g, rows, channels=channels, n=n, row_stride=rs)
    else:
        C.sampler_step_2m(x_d, eps_d, inp_d, hist_d, coef_d, tt_d, step_d, first_d, t_d, g, rows, n=n, row_stride=rs)
    assert int(step_d.item()) == n_steps and float(t_d.item()) == float(t_table[n_steps])
    _same(x_d, before[0], "state after a launch past the table")
    _same(inp_d, before[1], "input after a launch past the table")
    _same(hist_d, before[2], "history after a launch past the table")
    return orders


@pytest.mark.parametrize("first", [0, 2], ids=["first0", "first2"])
@pytest.mark.parametrize("n", [5, 8 * 1031, 8 * 1031 + 3], ids=["n5", "n8k", "n8k+3"])
@pytest.mark.parametrize("rows", [1, 2], ids=["rows1", "rows2"])
def test_step_2m_kernel_equals_the_restatement(C, rows, n, first):
    """A 6-step table from step `first`: the first executed step and the last are first-order, the others second-order;
    the body alone, body + tail and the tail alone."""
    from mixdq_amd.sampler import schedule
    s = schedule("dpmpp_2m", 6)
    for g in (7.5, 0.0) if rows == 2 else (0.0,):
        orders = _run_2m_steps(C, s, n, rows, g, seed=100 * rows + 10 * first + n % 7, first=first)
        assert orders == [False] + [True] * (4 - first) + [False]
    _run_2m_steps(C, schedule("dpmpp_2m", 6, karras=True), n, rows, 3.0, seed=n % 11 + first, first=first)


def test_step_2m_kernel_grid_stride(C):
    """More 8-element vectors than the launch has lanes (the grid is capped at 2048 workgroups of 256): the loop takes a
    second trip, on a second-order step (D2 != 0, the history is read) and on the last one."""
    from mixdq_amd.sampler import schedule
    s = schedule("dpmpp_2m", 4)
    assert s.coef[2, 5] != 0
    n = 8 * (2048 * 256 + 37) + 5
    assert _run_2m_steps(C, s, n, 2, 5.0, seed=3, first=0, start=2) == [True, False]


def test_step_2m_past_the_table_and_refusals(C):
    from mixdq_amd.sampler import schedule
    s = schedule("dpmpp_2m", 3)
    n = 64
    x_d, hist_d = t(np.arange(n, dtype=f32)), torch.full((n,), float("nan"), device=DEV)
    eps_d = t(np.ones(n, dtype=np.float16))
    inp_d = torch.full((n,), 3.0, dtype=torch.float16, device=DEV)
    step_d = torch.tensor([3], dtype=torch.int32, device=DEV)
    first_d = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_d = torch.tensor(5.0, device=DEV)
    args = [x_d, eps_d, inp_d, hist_d, t(s.coef), t(s.t_table), step_d, first_d, t_d]
    C.sampler_step_2m(*args)                                          # step == n_steps: past the table
    step_d.fill_(-1)
    C.sampler_step_2m(*args)
    assert int(step_d.item()) == -1 and float(t_d.item()) == 5.0
    assert torch.equal(x_d, t(np.arange(n, dtype=f32))) and bool((inp_d == 3.0).all()) and bool(hist_d.isnan().all())
    step_d.zero_()
    with pytest.raises(RuntimeError, match="invalid argument"):
        C.sampler_step_2m(*args, 0.0, 3)
    with pytest.raises(RuntimeError, match="invalid argument"):
        C.sampler_step_2m(x_d, eps_d, inp_d, x_d, *args[4:])          # the history may not be the state
    with pytest.raises(RuntimeError, match="alignment"):
        C.sampler_step_2m(x_d, eps_d, inp_d, hist_d[1:], *args[4:], n=32)
    with pytest.raises(RuntimeError, match="coef8 should be"):
        C.sampler_step_2m(*args[:4], t(schedule("euler", 3).coef), *args[5:])
    with pytest.raises(RuntimeError, match="first should be"):
        C.sampler_step_2m(*args[:7], first_d.float(), t_d)
    with pytest.raises(RuntimeError, match="hist is smaller"):
        C.sampler_step_2m(x_d, eps_d, inp_d, hist_d[:32], *args[4:])
    z_d = torch.zeros(n, device=DEV)
    with pytest.raises(RuntimeError, match="invalid argument"):
        C.sampler_step_2m_masked(*args, z_d, z_d, torch.ones(n // 4, device=DEV), t(s.blend), channels=3)
    with pytest.raises(RuntimeError, match="blend should be"):
        C.sampler_step_2m_masked(*args, z_d, z_d, torch.ones(n // 4, device=DEV), t(s.coef))
    assert int(step_d.item()) == 0 and float(t_d.item()) == 5.0 and bool((inp_d == 3.0).all())     # nothing ran
    assert bool(hist_d.isnan().all())


# n: the 8-element body alone, body + tail -- channels 4 (two mask values per pass) and 3 (the generic walk)
MASKED_SHAPES = [(4 * 8 * 8, 4), (4 * 3 * 5, 4), (3 * 7 * 5, 3), (3 * 8 * 8, 3)]


@pytest.mark.parametrize("mask_kind", ["zeros", "ones", "soft"])
@pytest.mark.parametrize("n,channels", MASKED_SHAPES, ids=[f"n{n}c{c}" for n, c in MASKED_SHAPES])
@pytest.mark.parametrize("rows", [1, 2], ids=["rows1", "rows2"])
def test_masked_step_2m_kernel_equals_the_restatement(C, rows, n, channels, mask_kind):
    from mixdq_amd.sampler import schedule
    s = schedule("dpmpp_2m", 4)
    g = 7.5 if rows == 2 else 0.0
    for first in (0, 1):
        orders = _run_2m_steps(C, s, n, rows, g, seed=10 * rows + n % 7 + first, first=first, channels=channels,
                               mask_kind=mask_kind)
        assert orders == [False] + [True] * (2 - first) + [False]


# ---- the loop ------------------------------------------------------------------------------------------------------
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


def _inputs(B, rows, seed):
    from mixdq_amd.quantize_sdxl import example_inputs
    inp = example_inputs(B * rows, L_TINY, DEV, seed=seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    noise = torch.randn(B, 4, L_TINY, L_TINY, generator=g).to(DEV)
    z = (torch.randn(B, 4, L_TINY, L_TINY, generator=g) * 0.13025).to(DEV)        # as VAEEncoder.encode leaves them
    mask = (torch.rand(B, L_TINY, L_TINY, generator=g) < 0.5).float().to(DEV)
    return z, noise, inp["encoder_hidden_states"], inp["added_cond_kwargs"], mask


def _eager(unet, sampler, noise, ehs, added, z=None, strength=None, mask=None):
    """The loop a user would have to write: the start state as Sampler builds it, then per step a UNet call, the
    restatement of the step (order 2: with the history carried along; the first executed step first-order), the
    blend's where there is a mask, and the FP16 input recomputed.  Returns (t0, state, last history)."""
    from mixdq_amd.sampler import img2img_start
    s, rows, g = sampler.schedule, sampler.rows_per_image, sampler.guidance_scale
    B = noise.shape[0]
    if strength is None:
        t0 = 0
        x, inp = R.init(noise.float().cpu().numpy(), s.init_scale, s.input_scale0)
    else:
        t0 = img2img_start(s.n_steps, strength)
        a0, c0, s0 = (torch.tensor(v, dtype=torch.float32, device=DEV) for v in s.start(t0))
        az = z.float() * a0                                  # three torch operations, each rounded to FP32
        cn = noise.float() * c0
        x = az + cn
        inp = (x * s0).to(torch.float16).cpu().numpy()
        x = x.cpu().numpy()
    if mask is not None:
        z_np, n0 = z.float().cpu().numpy(), noise.float().cpu().numpy()
        m = np.broadcast_to(mask.cpu().numpy().reshape(B, 1, L_TINY, L_TINY), x.shape)
    hist = None
    for i in range(t0, s.n_steps):
        sample = t(np.concatenate([inp] * rows, axis=0))
        with torch.no_grad():
            eps = unet(sample, torch.tensor(float(s.timesteps[i]), device=DEV), ehs, added)[0]
        eps = eps.float().cpu().numpy().astype(np.float16)
        eu, ec = eps[:B], (eps[B:] if rows == 2 else None)
        if s.order == 2:
            y, hist = M.step(x, hist, eu, ec, s.coef[i], g, M.is_second(s.coef[i], i, t0))
            s_next = s.coef[i, 6]
        else:
            y, _ = R.step(x, eu, ec, s.coef[i], g)
            s_next = s.coef[i, 3]
        x = y if mask is None else I.blend(y, z_np, n0, m, s.blend[i, 0], s.blend[i, 1])
        inp = M.scaled_input(x, s_next)
    return t0, x, hist


@pytest.mark.parametrize("kind,n_steps,g,karras", [("dpmpp_2m", 6, 0.0, False), ("dpmpp_2m", 6, 7.5, False),
                                                   ("dpmpp_2m", 6, 0.0, True), ("dpmpp_2m", 6, 7.5, True),
                                                   ("ddim", 4, 0.0, False)])
def test_sampler_equals_the_eager_loop(tiny_unet, kind, n_steps, g, karras):
    """Graph replay == the eager loop, text-to-image and image-to-image (strength 0.5: the run starts first-order at
    t0 = n_steps / 2, on a history the text-to-image run before it left behind)."""
    from mixdq_amd import Sampler
    sm = Sampler(tiny_unet, kind, n_steps, guidance_scale=g, karras=karras)
    rows = sm.rows_per_image
    assert rows == (2 if g > 1 else 1) and sm.schedule.order == (2 if kind == "dpmpp_2m" else 1)
    for seed, strength in ((21, None), (22, 0.5), (23, None)):
        z, noise, ehs, added, _ = _inputs(2, rows, seed)
        graph = sm._graph
        if strength is None:
            got = sm.sample(noise, ehs, added)
        else:
            got = sm.sample(noise, ehs, added, init_latents=z, strength=strength)
        assert graph is None or sm._graph is graph
        t0, want, hist = _eager(tiny_unet, sm, noise, ehs, added, z, strength)
        assert t0 == (0 if strength is None else n_steps // 2) and int(sm._step.item()) == n_steps
        assert got.dtype == torch.float32 and got.shape == noise.shape and bool(torch.isfinite(got).all())
        _same(got, want, f"{kind} x {n_steps} from step {t0}, seed {seed}")
        if sm.schedule.order == 2:
            assert int(sm._first.item()) == t0
            _same(sm._hist, hist, "the history the run leaves: the last step's x0")
            _same(got, hist, "the last step is x' = x0")


def test_one_multistep_sampler_serves_plain_img2img_and_masked_calls(tiny_unet):
    """plain -> img2img -> masked -> plain on one Sampler: each result equals a fresh Sampler's and the eager loop's
    (every run's first step ignores the history of the run before it)."""
    from mixdq_amd import Sampler
    z, noise, ehs, added, mask = _inputs(1, 1, 81)
    calls = {"plain": lambda s: s.sample(noise, ehs, added),
             "img2img": lambda s: s.sample(noise, ehs, added, init_latents=z, strength=0.5),
             "masked": lambda s: s.sample(noise, ehs, added, init_latents=z, strength=0.7, mask=mask)}
    eager = {"plain": {}, "img2img": dict(z=z, strength=0.5), "masked": dict(z=z, strength=0.7, mask=mask)}
    sm = Sampler(tiny_unet, "dpmpp_2m", 6)
    fresh = {}
    for k in ("plain", "img2img", "masked"):
        fresh[k] = calls[k](Sampler(tiny_unet, "dpmpp_2m", 6))
        _same(fresh[k], _eager(tiny_unet, sm, noise, ehs, added, **eager[k])[1], f"{k} on a fresh Sampler")
    for k in ("plain", "img2img", "masked", "plain", "masked", "img2img"):
        _same(calls[k](sm), fresh[k], f"{k} after other kinds of call")
    assert sm._graph is not None and sm._graph_masked is not None and sm._graph is not sm._graph_masked
    keep = (mask == 0)[:, None].expand_as(z)
    assert bool(keep.any()) and torch.equal(fresh["masked"][keep], z.float()[keep])   # the last blend row is (1, 0)
    assert not torch.equal(fresh["plain"], fresh["img2img"]) and not torch.equal(fresh["img2img"], fresh["masked"])
