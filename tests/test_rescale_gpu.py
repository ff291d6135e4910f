"""Guidance rescale on the GPU.  mixdq_sampler_step_rescaled bit for bit against tests/rescale_ref.py on top of the
existing restatements, over every instantiation of the statistics and step kernels and at the shapes where the
reduction can go wrong; its invariants against today's entry points (rescale 0, guidance 1, an image alone); and
Sampler(guidance_rescale=, prediction_type=, zero_snr=) bit-equal to an eager loop around the same UNet.

Every batch holds images of deliberately different mean and spread (one of them a mean of 64), so that a wrong image
index, a sum that cancels or a chunk counted twice shows in the factor."""
import numpy as np
import pytest
import torch

from tests import inpaint_ref as I
from tests import ip2p_ref as P
from tests import multistep_ref as M
from tests import rescale_ref as RR
from tests import rng_ref as G
from tests import sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_TINY = 32
f32 = np.float32
PAD = np.float16(-7.25)
G_T, G_I, PHI = 7.5, 1.5, 0.7
MEANS, SPREADS = (0.0, 64.0, -3.0), (1.0, 0.5, 2.0)

# n_image: 252 = 4*9*7 -- one partial chunk, no multiple of 8, element-by-element loads (NOISE 3); 2072 = 4*518 -- a full
# chunk + 24 elements (NOISE 2); 4096 -- two full chunks; 6400 = 4*40*40 -- three full chunks + 256; 65536 -- SDXL's
# latent size, 32 chunks, one image
SHAPES = {252: 3, 2072: 3, 4096: 3, 6400: 3, 65536: 1}
MODES = ("plain", "buffer", "seeds", "2m")


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


def _schedule(mode):
    from mixdq_amd.sampler import Schedule
    kind = {"plain": "euler", "buffer": "euler_ancestral", "seeds": "euler_ancestral", "2m": "dpmpp_2m"}[mode]
    return Schedule(kind, 3, prediction_type="v_prediction")


class _Case:
    """The operands of a launch on the host and on the device: `rows` row blocks at a padded stride, a sentinel in the
    gaps and behind the last block.  channels: 0 unmasked, else the mask's channel count."""

    def __init__(self, rows, n_image, B, mode, channels, seed, g=G_T, phi=PHI, images=None):
        self.rows, self.n_image, self.B, self.mode, self.ch = rows, n_image, B, mode, channels
        self.n = n = B * n_image
        self.g, self.gi, self.phi = g, G_I, phi
        self.sch = _schedule(mode)
        self.rs = _up(n, 8) + 8
        self.ns = _up(n, 4) + 4
        self.rng = rng = np.random.default_rng(seed)
        self.images = list(range(B)) if images is None else images       # which (mean, spread) each image carries
        self.x = (rng.standard_normal(n) * 3).astype(f32)
        self.hist = np.full(n, np.nan, dtype=f32) if mode == "2m" else None
        self.noise = rng.standard_normal((3, self.ns)).astype(f32) if mode == "buffer" else None
        self.seeds = [int(s) for s in rng.integers(0, 2 ** 62, B)] if mode == "seeds" else None
        if channels:
            self.z = rng.standard_normal(n).astype(f32)
            self.noise0 = rng.standard_normal(n).astype(f32)
            self.mask = rng.choice(np.array([0.0, 1.0, 0.25], dtype=f32), n // channels)

    def eps(self):
        """One step's model output: per image its own mean and spread in every row block."""
        e = np.full(self.rows * self.rs + 16, PAD, dtype=np.float16)
        for r in range(self.rows):
            for b, which in enumerate(self.images):
                v = self.rng.standard_normal(self.n_image) * SPREADS[which % 3] + MEANS[which % 3]
                at = r * self.rs + b * self.n_image
                e[at:at + self.n_image] = v.astype(np.float16)
        return e

    def blocks(self, e):
        return [e[r * self.rs:r * self.rs + self.n] for r in range(self.rows)]

    def device(self, C):
        self.x_d = t(self.x)
        self.coef_d, self.tt_d = t(self.sch.coef), t(self.sch.t_table)
        self.step_d = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.t_d = torch.tensor(-1.0, dtype=torch.float32, device=DEV)
        self.ws = C.sampler_rescale_workspace(self.n, self.n_image, DEV)
        self.ws.fill_(float("nan"))                        # nothing is read that this step did not write
        self.kw = dict(n=self.n, row_stride=self.rs)
        if self.mode == "buffer":
            self.kw.update(noise=t(self.noise), noise_stride=self.ns)
        if self.mode == "seeds":
            self.kw.update(seeds=torch.tensor(self.seeds, dtype=torch.int64, device=DEV))
        if self.mode == "2m":
            self.hist_d = t(self.hist)
            self.kw.update(hist=self.hist_d, first=torch.zeros(1, dtype=torch.int32, device=DEV))
        if self.ch:
            self.kw.update(z=t(self.z), noise0=t(self.noise0), mask=t(self.mask), blend=t(self.sch.blend),
                           channels=self.ch)
        return self

    def launch(self, C, e):
        inp_d = torch.full((self.rows * self.rs + 16,), float(PAD), dtype=torch.float16, device=DEV)
        C.sampler_step_rescaled(self.x_d, t(e), inp_d, self.coef_d, self.tt_d, self.step_d, self.t_d, self.g,
                                self.gi if self.rows == 3 else None, self.phi, self.ws, rows_per_image=self.rows,
                                n_image=self.n_image, **self.kw)
        return inp_d.cpu().numpy()

    def launch_sibling(self, C, e):
        """Today's entry point of the same mode (no rescale), on the same device state."""
        inp_d = torch.full((self.rows * self.rs + 16,), float(PAD), dtype=torch.float16, device=DEV)
        kw = dict(self.kw)
        if self.mode == "seeds":
            kw["n_image"] = self.n_image
        if self.rows == 3:
            C.sampler_step3(self.x_d, t(e), inp_d, self.coef_d, self.tt_d, self.step_d, self.t_d, self.g, self.gi, **kw)
            return inp_d.cpu().numpy()
        masked = [kw.pop(k) for k in ("z", "noise0", "mask", "blend")] if self.ch else []
        if self.mode == "2m":
            hist, first = kw.pop("hist"), kw.pop("first")
            fn = C.sampler_step_2m_masked if self.ch else C.sampler_step_2m
            fn(self.x_d, t(e), inp_d, hist, self.coef_d, self.tt_d, self.step_d, first, self.t_d, *masked, self.g, 2, **kw)
        else:
            noise = kw.pop("noise", None)
            fn = C.sampler_step_masked if self.ch else C.sampler_step
            fn(self.x_d, t(e), inp_d, self.coef_d, self.tt_d, self.step_d, self.t_d, *masked, self.g, 2, noise, **kw)
        return inp_d.cpu().numpy()

    def reference(self, i, blocks):
        """Step i of the restatement on the host state; returns (the FP16 input, the factors)."""
        row = self.sch.coef[i]
        noise = None
        if self.mode == "buffer":
            noise = self.noise[i, :self.n]
        if self.mode == "seeds":
            noise = np.concatenate([G.randn_image(s, self.n_image, 1, i) for s in self.seeds])
        blend = None
        if self.ch:
            blend = (self.z, self.noise0, np.repeat(self.mask, self.ch), self.sch.blend[i, 0], self.sch.blend[i, 1])
        second = self.mode == "2m" and M.is_second(row, i, 0)
        _, r = RR.rescaled(blocks, self.g, self.gi, self.phi, self.n_image)
        self.x, want_in, p0 = RR.step(self.x, blocks, row, self.g, self.gi, self.phi, self.n_image, noise=noise,
                                      hist=self.hist, second=second, blend=blend)
        if self.mode == "2m":
            self.hist = p0
        return want_in, r

    def check(self, got_in, want_in, what):
        n, rs = self.n, self.rs
        _same(self.x_d, self.x, f"{what}: state")
        if self.mode == "2m":
            _same(self.hist_d, self.hist, f"{what}: hist")
        for r in range(self.rows):
            _same(got_in[r * rs:r * rs + n], want_in, f"{what}: UNet input block {r}")
            assert (got_in[r * rs + n:(r + 1) * rs] == PAD).all(), f"{what}: the gap behind block {r} was written"
        assert (got_in[self.rows * rs:] == PAD).all(), f"{what}: written behind the last block"


def _three_steps(C, c, what):
    factors = []
    for i in range(3):                                  # 2m: a first-order step, a second-order one, the last
        e = c.eps()
        got_in = c.launch(C, e)
        want_in, r = c.reference(i, c.blocks(e))
        c.check(got_in, want_in, f"{what} step {i}")
        assert int(c.step_d.item()) == i + 1 and float(c.t_d.item()) == float(c.sch.t_table[i + 1])
        factors.append(r)
    assert np.isfinite(c.x).all()
    return np.stack(factors)


# ---- the kernels against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [0, 4, 3], ids=["unmasked", "mask4", "mask3"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_image", [252, 2072])
@pytest.mark.parametrize("rows", [2, 3])
def test_rescaled_step_equals_the_restatement(C, rows, n_image, mode, channels):
    c = _Case(rows, n_image, 3, mode, channels, seed=rows * 1000 + n_image + 7 * MODES.index(mode) + channels).device(C)
    r = _three_steps(C, c, f"rows {rows} n_image {n_image} {mode} channels {channels}")
    # the three images differ in spread and mean: so do their factors, and none is the trivial one
    assert (r != 1.0).all() and len(np.unique(r[0])) == 3
    assert 0.0 < r.min() and r.max() < 1.0              # guidance 7.5 widens the spread: rescale shrinks it back


@pytest.mark.parametrize("n_image", list(SHAPES))
@pytest.mark.parametrize("rows", [2, 3])
def test_plain_rescaled_step_at_every_chunk_count(C, rows, n_image):
    c = _Case(rows, n_image, SHAPES[n_image], "plain", 0, seed=rows + n_image).device(C)
    _three_steps(C, c, f"rows {rows} n_image {n_image}")
    chunks = (n_image + RR.CHUNK - 1) // RR.CHUNK
    assert c.ws.numel() == SHAPES[n_image] * (4 * chunks + 1)
    stats = c.ws[:4 * SHAPES[n_image] * chunks]
    assert bool(torch.isfinite(stats).all()), "a chunk's statistics were not written"


def test_2m_at_sdxl_size(C):
    c = _Case(2, 65536, 1, "2m", 4, seed=5, images=[1]).device(C)
    _three_steps(C, c, "sdxl 2m masked")


# ---- invariants against today's entry points ----------------------------------------------------------------------
@pytest.mark.parametrize("channels", [0, 4], ids=["unmasked", "mask4"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_image", [252, 2072])
@pytest.mark.parametrize("rows", [2, 3])
def test_rescale_zero_is_todays_step(C, rows, n_image, mode, channels):
    seed = 31 * rows + n_image + MODES.index(mode) + channels
    a = _Case(rows, n_image, 3, mode, channels, seed, phi=0.0).device(C)
    b = _Case(rows, n_image, 3, mode, channels, seed, phi=0.0).device(C)
    for i in range(3):
        e = a.eps()
        assert np.array_equal(_bits(e), _bits(b.eps()))
        got, want = a.launch(C, e), b.launch_sibling(C, e)
        _same(got, want, f"step {i}: UNet input")
        _same(a.x_d, b.x_d, f"step {i}: state")
        if mode == "2m":
            _same(a.hist_d, b.hist_d, f"step {i}: hist")
        assert int(a.step_d.item()) == int(b.step_d.item()) == i + 1 and float(a.t_d.item()) == float(b.t_d.item())


@pytest.mark.parametrize("phi", [0.3, 1.0])
@pytest.mark.parametrize("mode", ["plain", "seeds", "2m"])
def test_guidance_one_is_the_plain_step_for_any_phi(C, mode, phi):
    """Two rows at guidance 1: e = u + (c - u).  On values that are multiples of 2^-6 below 16 both operations are exact,
    e == c element for element, the two sums of squares are the same number and r == 1 exactly."""
    a = _Case(2, 2072, 3, mode, 0, seed=77, g=1.0, phi=phi).device(C)
    b = _Case(2, 2072, 3, mode, 0, seed=77, g=1.0, phi=phi).device(C)
    for i in range(3):
        e = a.eps()
        b.eps()
        e = (np.clip(np.rint(e.astype(f32) * 64), -1023, 1023) / 64).astype(np.float16)
        _same(a.launch(C, e), b.launch_sibling(C, e), f"step {i}: UNet input")
        _same(a.x_d, b.x_d, f"step {i}: state")


@pytest.mark.parametrize("channels", [0, 4], ids=["unmasked", "mask4"])
@pytest.mark.parametrize("mode", ["plain", "seeds", "2m"])
@pytest.mark.parametrize("n_image", [252, 6400])
@pytest.mark.parametrize("rows", [2, 3])
def test_every_image_of_a_batch_equals_the_image_alone(C, rows, n_image, mode, channels):
    seed = 5 * rows + n_image + MODES.index(mode) + channels
    batch = _Case(rows, n_image, 3, mode, channels, seed).device(C)
    e = batch.eps()
    got_in = batch.launch(C, e)
    got_x = batch.x_d.cpu().numpy()
    for b in range(3):
        sl = slice(b * n_image, (b + 1) * n_image)
        one = _Case(rows, n_image, 1, mode, channels, seed, images=[b])
        one.x = batch.x[sl].copy()
        if mode == "seeds":
            one.seeds = [batch.seeds[b]]
        if channels:
            one.z, one.noise0 = batch.z[sl].copy(), batch.noise0[sl].copy()
            one.mask = batch.mask[b * n_image // channels:(b + 1) * n_image // channels].copy()
        one.device(C)
        e1 = np.full(rows * one.rs + 16, PAD, dtype=np.float16)
        for r in range(rows):
            e1[r * one.rs:r * one.rs + n_image] = e[r * batch.rs + b * n_image:r * batch.rs + (b + 1) * n_image]
        in1 = one.launch(C, e1)
        _same(one.x_d, got_x[sl], f"image {b}: state")
        _same(in1[:n_image], got_in[sl], f"image {b}: UNet input")
        if mode == "2m":
            _same(one.hist_d, batch.hist_d[sl], f"image {b}: hist")


def test_past_the_table_nothing_is_written(C):
    c = _Case(2, 2072, 3, "2m", 4, seed=9).device(C)
    c.step_d.fill_(3)
    e = c.eps()
    got_in = c.launch(C, e)
    assert (got_in == PAD).all() and int(c.step_d.item()) == 3 and float(c.t_d.item()) == -1.0
    _same(c.x_d, c.x, "state")
    assert bool(torch.isnan(c.ws).all()) and bool(torch.isnan(c.hist_d).all())


def test_binding_refusals(C):
    c = _Case(2, 252, 3, "plain", 0, seed=1).device(C)
    e, inp = t(c.eps()), torch.zeros(2 * c.rs + 16, dtype=torch.float16, device=DEV)
    head = (c.x_d, e, inp, c.coef_d, c.tt_d, c.step_d, c.t_d, G_T, None)
    for bad in (dict(phi=1.5), dict(phi=-0.1), dict(rows=1), dict(n_image=250), dict(ws=c.ws[:4]),
                dict(ws=c.ws.double())):
        with pytest.raises(RuntimeError):
            C.sampler_step_rescaled(*head, bad.get("phi", PHI), bad.get("ws", c.ws), rows_per_image=bad.get("rows", 2),
                                    n_image=bad.get("n_image", 252), **c.kw)
    assert int(c.step_d.item()) == 0


# ---- the loop ----------------------------------------------------------------------------------------------------
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
    z = (torch.randn(B, 4, L_TINY, L_TINY, generator=g) * 0.13025).to(DEV)
    mask = (torch.rand(B, L_TINY, L_TINY, generator=g) < 0.5).float().to(DEV)
    return z, noise, inp["encoder_hidden_states"], inp["added_cond_kwargs"], mask


def _storage(a):
    """[B, C, H, W] tensor -> numpy [B, H * W * C]: the values in storage (channels-last) order."""
    return a.detach().permute(0, 2, 3, 1).contiguous().cpu().numpy().reshape(a.shape[0], -1)


def _eager(unet, sampler, noise, ehs, added, z=None, mask=None, step_noise=None):
    """The loop a user would have to write, on the values in storage order: per step a UNet call at rows * B rows, then
    the restatement of the rescaled step."""
    s, rows, g, gi = sampler.schedule, sampler.rows_per_image, sampler.guidance_scale, sampler.image_guidance_scale
    B, Cc, H, W = noise.shape
    n_image = Cc * H * W
    x, inp = R.init(_storage(noise.float()).reshape(-1), s.init_scale, s.input_scale0)
    blend_ops = None
    if mask is not None:
        blend_ops = (_storage(z.float()).reshape(-1), _storage(noise.float()).reshape(-1),
                     np.repeat(mask.cpu().numpy().reshape(-1), Cc))
    hist = None
    for i in range(s.n_steps):
        sample = t(np.concatenate([inp.reshape(B, H, W, Cc)] * rows, axis=0)).permute(0, 3, 1, 2)
        with torch.no_grad():
            eps = unet(sample, torch.tensor(float(s.timesteps[i]), device=DEV), ehs, added)[0]
        eps = _storage(eps).astype(np.float16)
        blocks = [eps[r * B:(r + 1) * B].reshape(-1) for r in range(rows)]
        blend = None if mask is None else blend_ops + (s.blend[i, 0], s.blend[i, 1])
        sn = None if step_noise is None else _storage(step_noise[i]).reshape(-1)
        x, inp, hist = RR.step(x, blocks, s.coef[i], g, gi, sampler.guidance_rescale, n_image, noise=sn, hist=hist,
                               second=s.order == 2 and M.is_second(s.coef[i], i, 0), blend=blend)
    return x.reshape(B, H, W, Cc).transpose(0, 3, 1, 2)


KINDS = {"euler": dict(kind="euler"), "dpmpp_2m": dict(kind="dpmpp_2m"),
         "ddim_zero_snr": dict(kind="ddim", spacing="trailing", zero_snr=True)}


@pytest.mark.parametrize("rows", [2, 3])
@pytest.mark.parametrize("name", list(KINDS))
def test_rescaled_sampler_equals_the_eager_loop(C, tiny_unet, name, rows):
    from mixdq_amd import Sampler
    kw = dict(KINDS[name], prediction_type="v_prediction", guidance_rescale=PHI)
    if rows == 3:
        kw["image_guidance_scale"] = G_I
    sm = Sampler(tiny_unet, kw.pop("kind"), 3, G_T, **kw)
    assert sm.rows_per_image == rows
    graphs, results = None, []
    for seed in (51, 52):                                          # other inputs: the same graph objects
        z, noise, ehs, added, mask = _inputs(2, rows, seed)
        got = sm.sample(noise, ehs, added)
        now = (sm._graph, sm._graph_masked, sm._graph_rng, sm._graph_masked_rng)
        assert sum(gr is not None for gr in now) == 1 and (graphs is None or now == graphs), "one graph, never re-captured"
        graphs = now
        assert sm._step_binding == "sampler_step_rescaled"
        assert got.dtype == torch.float32 and got.shape == noise.shape and bool(torch.isfinite(got).all())
        _same(got, _eager(tiny_unet, sm, noise, ehs, added), f"{name} rows {rows}, inputs {seed}")
        results.append(got)
    assert not torch.equal(results[0], results[1])
    # masked: a second graph on the same buffers, the first untouched
    got = sm.sample(noise, ehs, added, init_latents=z, mask=mask)
    assert sm._graph is graphs[0] and sm._graph_masked is not None
    _same(got, _eager(tiny_unet, sm, noise, ehs, added, z=z, mask=mask), "masked")
    # seeded: the start noise made on the device, the same plain graph
    shape = tuple(noise.shape)
    got = sm.sample(shape, ehs, added, seed=11)
    start = C.randn(shape, torch.tensor([11, 12], dtype=torch.int64, device=DEV))
    _same(got, _eager(tiny_unet, sm, start, ehs, added), "seeded")
    assert sm._graph is graphs[0]
    # the rescale matters, and so does the prediction type
    kw0 = dict(kw, guidance_rescale=0.0)
    plain = Sampler(tiny_unet, KINDS[name]["kind"], 3, G_T, **kw0)
    assert not torch.equal(plain.sample(noise, ehs, added), sm.sample(noise, ehs, added))


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_rescaled_stochastic_sampler_with_seeds(C, tiny_unet, masked):
    """'euler_ancestral': the steps compute their noise in registers (the _rng graphs) behind the rescale."""
    from mixdq_amd import Sampler
    sm = Sampler(tiny_unet, "euler_ancestral", 3, G_T, prediction_type="v_prediction", guidance_rescale=PHI)
    z, noise, ehs, added, mask = _inputs(2, 2, 71)
    shape = tuple(noise.shape)
    sd = torch.tensor([21, 22], dtype=torch.int64, device=DEV)
    extra = dict(init_latents=z, mask=mask) if masked else {}
    got = sm.sample(shape, ehs, added, seed=21, **extra)
    assert (sm._graph_masked_rng if masked else sm._graph_rng) is not None and sm._step_binding == "sampler_step_rescaled"
    start = C.randn(shape, sd)
    sn = torch.stack([C.randn(shape, sd, C.RNG_STREAM_STEP, i) for i in range(3)])
    want = _eager(tiny_unet, sm, start, ehs, added, step_noise=sn, **(dict(z=z, mask=mask) if masked else {}))
    _same(got, want, "seeded ancestral")


@pytest.mark.parametrize("cfg,binding", [(dict(kind="euler"), "sampler_step"), (dict(kind="dpmpp_2m"), "sampler_step_2m"),
                                         (dict(kind="euler", image_guidance_scale=G_I), "sampler_step3")],
                         ids=["euler", "dpmpp_2m", "three_rows"])
def test_without_rescale_the_captured_binding_is_todays(C, tiny_unet, cfg, binding):
    from mixdq_amd import Sampler
    cfg = dict(cfg)
    sm = Sampler(tiny_unet, cfg.pop("kind"), 2, G_T, **cfg)
    z, noise, ehs, added, mask = _inputs(2, sm.rows_per_image, 81)
    sm.sample(noise, ehs, added)
    assert sm._step_binding == binding and not hasattr(sm, "_rescale_ws")
    sm.sample(noise, ehs, added, init_latents=z, mask=mask)
    assert sm._step_binding == {"sampler_step": "sampler_step_masked", "sampler_step_2m": "sampler_step_2m_masked",
                                "sampler_step3": "sampler_step3"}[binding]
