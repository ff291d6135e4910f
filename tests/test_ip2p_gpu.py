"""InstructPix2Pix on the GPU.  mixdq_sampler_step3 bit for bit against its numpy restatement (tests/ip2p_ref.py on top
of the existing ones) over every instantiation of the step template it can reach, tied to the two-row kernel where the
image-only and unconditional rows coincide, and past the table; mixdq_ip2p_cond_f16 against its restatement;
Sampler(image_guidance_scale=) bit-equal to an eager loop that calls the UNet at 3B rows and then the restatement; and
Sampler.instruct against its parts done by hand."""
import numpy as np
import pytest
import torch

from tests import inpaint_ref as I
from tests import ip2p_ref as P
from tests import multistep_ref as M
from tests import rng_ref as G
from tests import sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_TINY = 32
f32 = np.float32
PAD = np.float16(-7.25)


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


# ---- the step kernel ---------------------------------------------------------------------------------------------
# (B, channels, h, w): n = 420 -- 52 passes and a tail of 4, n_image % 8 != 0 (NOISE 3), MASK 1; n_image = 64 (NOISE 2),
# MASK 1, no tail; channels 3 (MASK 2), tail of 2, NOISE 3; channels 3 with n_image = 24 (NOISE 2 with MASK 2)
SHAPES = {"3x4x5x7": (3, 4, 5, 7), "2x4x4x4": (2, 4, 4, 4), "2x3x5x7": (2, 3, 5, 7), "2x3x2x4": (2, 3, 2, 4)}
MODES = ("plain", "buffer", "seeds", "2m")
G_T, G_I = 7.5, 1.5


def _schedule(mode):
    from mixdq_amd.sampler import Schedule
    return Schedule({"plain": "euler", "buffer": "euler_ancestral", "seeds": "euler_ancestral", "2m": "dpmpp_2m"}[mode], 3)


class _Case:
    """The operands of a three-row launch on the host and on the device; row blocks at a padded stride, a sentinel in
    the gaps and behind the third block."""

    def __init__(self, shape, mode, masked, seed, start=0, g=G_T, gi=G_I):
        self.B, self.ch, h, w = shape
        self.n_image = self.ch * h * w
        self.n = n = self.B * self.n_image
        self.mode, self.masked, self.g, self.gi = mode, masked, g, gi
        self.sch = _schedule(mode)
        self.rs = _up(n, 8) + 8
        self.rng = rng = np.random.default_rng(seed)
        self.x = (rng.standard_normal(n) * 3).astype(f32)
        self.hist = np.full(n, np.nan, dtype=f32) if mode == "2m" else None        # not read on a first-order step
        self.start = start
        self.ns = _up(n, 4) + 4                          # the noise blocks at a padded stride too
        self.noise = rng.standard_normal((3, self.ns)).astype(f32) if mode == "buffer" else None
        self.seeds = [int(s) for s in rng.integers(0, 2 ** 62, self.B)] if mode == "seeds" else None
        if masked:
            self.z = rng.standard_normal(n).astype(f32)
            self.noise0 = rng.standard_normal(n).astype(f32)
            self.mask = rng.choice(np.array([0.0, 1.0, 0.25], dtype=f32), n // self.ch)
        # device
        self.x_d = t(self.x)
        self.coef_d, self.tt_d = t(self.sch.coef), t(self.sch.t_table)
        self.step_d = torch.tensor([start], dtype=torch.int32, device=DEV)
        self.t_d = torch.tensor(-1.0, dtype=torch.float32, device=DEV)
        self.kw = dict(n=n, row_stride=self.rs)
        if mode == "buffer":
            self.kw.update(noise=t(self.noise), noise_stride=self.ns)
        if mode == "seeds":
            self.kw.update(seeds=torch.tensor(self.seeds, dtype=torch.int64, device=DEV), n_image=self.n_image)
        if mode == "2m":
            self.hist_d = t(self.hist)
            self.kw.update(hist=self.hist_d, first=torch.tensor([start], dtype=torch.int32, device=DEV))
        if masked:
            self.kw.update(z=t(self.z), noise0=t(self.noise0), mask=t(self.mask), blend=t(self.sch.blend),
                           channels=self.ch)

    def eps(self):
        e = self.rng.standard_normal(3 * self.rs + 16).astype(np.float16)
        return e, [e[r * self.rs:r * self.rs + self.n] for r in range(3)]

    def launch(self, C, eps):
        inp_d = torch.full((3 * self.rs + 16,), float(PAD), dtype=torch.float16, device=DEV)
        C.sampler_step3(self.x_d, t(eps), inp_d, self.coef_d, self.tt_d, self.step_d, self.t_d, self.g, self.gi,
                        **self.kw)
        return inp_d.cpu().numpy()

    def reference(self, i, blocks):
        """Step i of the restatement on the host state; returns the FP16 input."""
        row = self.sch.coef[i]
        noise = None
        if self.mode == "buffer":
            noise = self.noise[i, :self.n]
        if self.mode == "seeds":
            noise = np.concatenate([G.randn_image(s, self.n_image, 1, i) for s in self.seeds])
        blend = None
        if self.masked:
            blend = (self.z, self.noise0, np.repeat(self.mask, self.ch), self.sch.blend[i, 0], self.sch.blend[i, 1])
        second = self.mode == "2m" and M.is_second(row, i, self.start)
        self.x, want_in, p0 = P.step3(self.x, *blocks, row, self.g, self.gi, noise=noise, hist=self.hist, second=second,
                                      blend=blend)
        if self.mode == "2m":
            self.hist = p0
        return want_in

    def check(self, got_in, want_in, what):
        n, rs = self.n, self.rs
        _same(self.x_d, self.x, f"{what}: state")
        if self.mode == "2m":
            _same(self.hist_d, self.hist, f"{what}: hist")
        for r in range(3):
            _same(got_in[r * rs:r * rs + n], want_in, f"{what}: UNet input block {r}")
            assert (got_in[r * rs + n:(r + 1) * rs] == PAD).all(), f"{what}: the gap behind block {r} was written"
        assert (got_in[3 * rs:] == PAD).all(), f"{what}: written behind the third block"


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_three_row_step_equals_the_restatement(C, shape, mode, masked):
    c = _Case(SHAPES[shape], mode, masked, seed=len(shape) * 7 + MODES.index(mode) * 3 + masked)
    assert c.rs % 8 == 0 and c.rs >= c.n + 8
    for i in range(3):                                  # 2m: a first-order step, a second-order one, the last
        eps, blocks = c.eps()
        got_in = c.launch(C, eps)
        want_in = c.reference(i, blocks)
        c.check(got_in, want_in, f"{shape} {mode} masked={masked} step {i}")
        assert int(c.step_d.item()) == i + 1 and float(c.t_d.item()) == float(c.sch.t_table[i + 1])
    assert np.isfinite(c.x).all()
    if mode == "2m":
        assert M.is_second(c.sch.coef[1], 1, 0) and not M.is_second(c.sch.coef[0], 0, 0)


@pytest.mark.parametrize("mode", ["buffer", "masked", "2m", "2m_masked"])
@pytest.mark.parametrize("gi", [1.5, -40.0])
def test_three_rows_with_equal_image_and_unconditional_blocks_are_the_two_row_kernel(C, mode, gi):
    masked, kind = "masked" in mode, "2m" if "2m" in mode else "buffer"
    c = _Case(SHAPES["3x4x5x7"], kind, masked, seed=77, start=0, gi=gi)
    n, rs = c.n, c.rs
    x2_d = c.x_d.clone()
    step2 = c.step_d.clone()
    t2 = c.t_d.clone()
    hist2 = c.hist_d.clone() if kind == "2m" else None
    for i in range(2):
        eps, blocks = c.eps()
        eps[rs:rs + n] = eps[2 * rs:2 * rs + n]           # block 1 a bit copy of block 2
        got3 = c.launch(C, eps)
        eps2 = np.concatenate([eps[2 * rs:3 * rs], eps[:rs]])            # (unconditional, conditional)
        inp2 = torch.full((2 * rs,), float(PAD), dtype=torch.float16, device=DEV)
        m = (c.kw["z"], c.kw["noise0"], c.kw["mask"], c.kw["blend"]) if masked else ()
        if kind == "2m":
            fn = C.sampler_step_2m_masked if masked else C.sampler_step_2m
            fn(x2_d, t(eps2), inp2, hist2, c.coef_d, c.tt_d, step2, c.kw["first"], t2, *m, c.g, 2, n=n, row_stride=rs,
               **(dict(channels=c.ch) if masked else {}))
        elif masked:
            C.sampler_step_masked(x2_d, t(eps2), inp2, c.coef_d, c.tt_d, step2, t2, *m, c.g, 2, c.kw["noise"],
                                  channels=c.ch, n=n, row_stride=rs, noise_stride=c.ns)
        else:
            C.sampler_step(x2_d, t(eps2), inp2, c.coef_d, c.tt_d, step2, t2, c.g, 2, c.kw["noise"], n=n, row_stride=rs,
                           noise_stride=c.ns)
        assert np.array_equal(c.x_d.cpu().numpy(), x2_d.cpu().numpy()), f"{mode} step {i}: state"
        got2 = inp2.cpu().numpy()
        for r in range(3):
            assert np.array_equal(got3[r * rs:r * rs + n], got2[:n]), f"{mode} step {i}: input block {r}"
        if kind == "2m":
            assert np.array_equal(c.hist_d.cpu().numpy(), hist2.cpu().numpy()), f"{mode} step {i}: hist"
        assert int(c.step_d.item()) == int(step2.item()) == i + 1


@pytest.mark.parametrize("mode", ["plain", "2m"])
def test_three_row_step_past_the_table_writes_nothing(C, mode):
    c = _Case(SHAPES["3x4x5x7"], mode, True, seed=5, start=3)          # the step index at n_steps
    if mode == "2m":
        c.hist[:] = 2.5
        c.hist_d.copy_(t(c.hist))
    eps, _ = c.eps()
    got_in = c.launch(C, eps)
    _same(c.x_d, c.x, "state")
    assert (got_in == PAD).all(), "an input was written"
    if mode == "2m":
        _same(c.hist_d, c.hist, "hist")
    assert int(c.step_d.item()) == 3 and float(c.t_d.item()) == -1.0


def test_three_row_binding_refusals(C):
    c = _Case(SHAPES["2x4x4x4"], "plain", False, seed=6)
    eps, _ = c.eps()
    inp = torch.zeros(3 * c.rs, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="smaller than rows_per_image row blocks"):
        C.sampler_step3(c.x_d, t(eps), inp[:2 * c.rs], c.coef_d, c.tt_d, c.step_d, c.t_d, 7.5, 1.5, **c.kw)
    with pytest.raises(RuntimeError, match="sampler_step3"):
        C.sampler_step3(c.x_d, t(eps), inp, c.coef_d, c.tt_d, c.step_d, c.t_d, 7.5, 1.5, n=c.n, row_stride=c.n - 8)
    with pytest.raises(RuntimeError, match="sampler_step:"):             # the two-row entry points keep refusing three
        C.sampler_step(c.x_d, t(eps), inp, c.coef_d, c.tt_d, c.step_d, c.t_d, 7.5, 3, n=c.n, row_stride=c.rs)
    assert int(c.step_d.item()) == 0


# ---- the conditioning kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 3, 8])
@pytest.mark.parametrize("rows", [1, 3])
def test_ip2p_cond_equals_the_restatement(C, rows, L):
    B, h, w = 2, 3, 5
    rng = np.random.default_rng(rows * 10 + L)
    m = (rng.standard_normal((B, h, w, 2 * L)) * 4).astype(np.float16)
    flat = m.reshape(-1, 2 * L)
    flat[:5, 0] = np.array([0.0, -0.0, 6e-8, 65504.0, -65504.0], dtype=np.float16)     # +-0, a subnormal, +-max
    flat[5:10, L - 1] = flat[:5, 0]
    assert flat[2, 0] != 0 and np.abs(flat[2, 0]) < 6.2e-5
    md = t(m).permute(0, 3, 1, 2)
    for scale in (1.0, 0.13025, 0.18215, -2.0):
        got = C.ip2p_cond(md, rows, scale)
        assert got.dtype == torch.float16 and tuple(got.shape) == (rows * B, 8, h, w)
        assert got.permute(0, 2, 3, 1).is_contiguous()
        got = got.permute(0, 2, 3, 1)
        _same(got, P.ip2p_cond(m, rows, scale), f"rows {rows} L {L} scale {scale}")
        gb = _bits(got)
        assert not gb[..., L:].any(), "padding channels are +0.0, sign bit included"
        if rows == 3:
            assert not gb[2 * B:].any(), "the third block is +0.0, sign bit included"
            assert np.array_equal(gb[:B], gb[B:2 * B])
        if scale == 1.0:
            assert np.array_equal(gb[:B, ..., :L], m[..., :L].view(np.uint16)), "scale 1.0 returns the mean's own bits"
    if L == 4:                                           # the moments at a 2-byte offset: the scalar loads
        big = torch.zeros(B * h * w * 8 + 1, dtype=torch.float16, device=DEV)
        off = big[1:].view(B, h, w, 8)
        off.copy_(t(m))
        _same(C.ip2p_cond(off.permute(0, 3, 1, 2), rows, 0.13025).permute(0, 2, 3, 1), P.ip2p_cond(m, rows, 0.13025),
              "moments at a 2-byte offset")
    assert tuple(C.ip2p_cond(md[:0], rows).shape) == (0, 8, h, w)


def test_ip2p_cond_refusals(C):
    m = torch.zeros((2, 4, 5, 8), dtype=torch.float16, device=DEV).permute(0, 3, 1, 2)
    with pytest.raises(RuntimeError, match="rows should be 1 or 3"):
        C.ip2p_cond(m, 2)
    with pytest.raises(RuntimeError, match="moments should be"):
        C.ip2p_cond(m.float())
    with pytest.raises(RuntimeError, match="moments should be"):
        C.ip2p_cond(m.contiguous())                                     # NCHW storage
    with pytest.raises(RuntimeError, match="1 to 8 latent channels"):
        C.ip2p_cond(torch.zeros((1, 2, 2, 18), dtype=torch.float16, device=DEV).permute(0, 3, 1, 2))


# ---- the loop ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny8(C):
    """The tiny W8A8 UNet of tests/test_inpaint9_gpu.py's recipe with an 8-channel conv_in (latent 32).  conv_in stays out
    of the activation config: the split needs it as a floating-point layer."""
    import bench
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet, quantizable_layers
    unet = build_unet(DEV, cfg=dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64, in_channels=8))
    inputs = example_inputs(2, L_TINY, DEV, in_channels=8, seed=7)
    ckpt = calibrate(unet, [inputs])
    bos_dict = precompute_bos(unet, inputs["encoder_hidden_states"])
    names = list(quantizable_layers(unet))
    act = {n: 8 for n in names if n not in ("conv_out", "conv_in")}
    quantize_unet(unet, bench.Cfg({n: 8 for n in names}, act), ckpt, bos=True, bos_dict=bos_dict)
    unet.set_fused(True)
    assert unet.cond_channels == 4 and not unet.conv_in.valid_for_acceleration
    assert unet.conv_in.weight.dtype == torch.float16 and tuple(unet.conv_in.weight.shape)[1] == 8
    yield unet
    del unet
    torch.cuda.empty_cache()


def _inputs(B, rows, seed, n_steps, uses_noise, C):
    from mixdq_amd.quantize_sdxl import example_inputs
    inp = example_inputs(B * rows, L_TINY, DEV, seed=seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    noise = torch.randn(B, 4, L_TINY, L_TINY, generator=g).to(DEV)
    z = (torch.randn(B, 4, L_TINY, L_TINY, generator=g) * 0.13025).to(DEV)
    step_noise = torch.randn(n_steps, B, 4, L_TINY, L_TINY, generator=g).to(DEV) if uses_noise else None
    mask = (torch.rand(B, L_TINY, L_TINY, generator=g) < 0.5).float().to(DEV)
    moments = (torch.randn(B, L_TINY, L_TINY, 8, generator=g) * 3).to(torch.float16).to(DEV).permute(0, 3, 1, 2)
    return z, noise, inp["encoder_hidden_states"], inp["added_cond_kwargs"], step_noise, mask, C.ip2p_cond(moments, rows)


def _eager(unet, sampler, noise, ehs, added, cond, step_noise=None, z=None, mask=None):
    """The loop a user would have to write: unet.cond_term once, then per step a UNet call at rows * B rows with
    cond_term=, the guidance's and the step's restatement, the blend's where there is a mask."""
    s, rows, g, gi = sampler.schedule, sampler.rows_per_image, sampler.guidance_scale, sampler.image_guidance_scale
    B = noise.shape[0]
    term = unet.cond_term(cond)
    if term.shape[0] != B * rows:
        term = torch.cat([term] * rows, dim=0).contiguous(memory_format=torch.channels_last)
    x, inp = R.init(noise.float().cpu().numpy(), s.init_scale, s.input_scale0)
    if mask is not None:
        z_np, n0 = z.float().cpu().numpy(), noise.float().cpu().numpy()
        m = np.broadcast_to(mask.cpu().numpy().reshape(B, 1, L_TINY, L_TINY), x.shape)
    hist = None
    for i in range(s.n_steps):
        sample = t(np.concatenate([inp] * rows, axis=0))
        with torch.no_grad():
            eps = unet(sample, torch.tensor(float(s.timesteps[i]), device=DEV), ehs, added, cond_term=term)[0]
        eps = eps.float().cpu().numpy().astype(np.float16)
        blend = None if mask is None else (z_np, n0, m, s.blend[i, 0], s.blend[i, 1])
        sn = step_noise[i].float().cpu().numpy() if s.uses_noise else None
        if rows == 3:
            x, inp, hist = P.step3(x, eps[:B], eps[B:2 * B], eps[2 * B:], s.coef[i], g, gi, noise=sn, hist=hist,
                                   second=s.order == 2 and M.is_second(s.coef[i], i, 0), blend=blend)
        else:
            y, _ = R.step(x, eps[:B], eps[B:] if rows == 2 else None, s.coef[i], g, sn)
            x = y if mask is None else I.blend(y, *blend)
            inp = M.scaled_input(x, s.coef[i, 3])
    return x


CALLS = {"euler": ("euler", {}), "ancestral_seed": ("euler_ancestral", {"seed": 11}), "dpmpp_2m": ("dpmpp_2m", {})}


@pytest.mark.parametrize("call", list(CALLS))
def test_three_row_sampler_equals_the_eager_loop(C, tiny8, call):
    from mixdq_amd import Sampler
    kind, extra = CALLS[call]
    sm = Sampler(tiny8, kind, 3, 7.5, image_guidance_scale=1.5)
    assert sm.rows_per_image == 3
    graphs, results = None, []
    for seed in (51, 52):                                         # two different cond on one Sampler
        z, noise, ehs, added, sn, mask, cond = _inputs(2, 3, seed, 3, False, C)
        assert tuple(cond.shape) == (6, 8, L_TINY, L_TINY) and tuple(ehs.shape)[0] == 6
        if "seed" in extra:
            shape = tuple(noise.shape)
            sd = torch.tensor([extra["seed"], extra["seed"] + 1], dtype=torch.int64, device=DEV)
            got = sm.sample(shape, ehs, added, seed=extra["seed"], cond=cond)
            noise = C.randn(shape, sd)
            sn = torch.stack([C.randn(shape, sd, C.RNG_STREAM_STEP, i) for i in range(3)])
        else:
            got = sm.sample(noise, ehs, added, cond=cond)
        now = (sm._graph, sm._graph_masked, sm._graph_rng, sm._graph_masked_rng)
        assert sum(gr is not None for gr in now) == 1 and (graphs is None or now == graphs), "one graph, never re-captured"
        graphs = now
        want = _eager(tiny8, sm, noise, ehs, added, cond, sn)
        assert got.dtype == torch.float32 and got.shape == noise.shape and bool(torch.isfinite(got).all())
        _same(got, want, f"{call}, inputs {seed}")
        results.append(got)
    assert not torch.equal(results[0], results[1])
    if call == "euler":
        # a masked call on the same Sampler: a second graph, the first untouched
        got = sm.sample(noise, ehs, added, init_latents=z, mask=mask, cond=cond)
        assert sm._graph is graphs[0] and sm._graph_masked is not None
        _same(got, _eager(tiny8, sm, noise, ehs, added, cond, z=z, mask=mask), "masked")
        _same(sm.sample(noise, ehs, added, cond=cond), results[1], "plain again after the masked call")
        # the image guidance matters: another scale, another result
        other = Sampler(tiny8, kind, 3, 7.5, image_guidance_scale=1.0).sample(noise, ehs, added, cond=cond)
        assert not torch.equal(other, results[1])


def test_two_row_sampler_on_the_same_unet_is_unchanged(C, tiny8):
    from mixdq_amd import Sampler
    sm = Sampler(tiny8, "euler", 3, 7.5)
    assert sm.rows_per_image == 2 and sm.image_guidance_scale is None
    _, noise, ehs, added, _, _, cond = _inputs(2, 1, 61, 3, False, C)
    from mixdq_amd.quantize_sdxl import example_inputs
    inp = example_inputs(4, L_TINY, DEV, seed=62)
    ehs, added = inp["encoder_hidden_states"], inp["added_cond_kwargs"]
    got = sm.sample(noise, ehs, added, cond=cond)                  # B rows of cond serve both row blocks
    _same(got, _eager(tiny8, sm, noise, ehs, added, cond), "two rows")


# ---- instruct() --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vaes(C):
    from mixdq_amd import vae as V
    cfg = dict(V.VAE_SDXL_CONFIG, block_out_channels=(32, 64, 128, 512), layers_per_block=1, norm_num_groups=8)
    return V.build_vae_encoder(cfg, seed=11, device=DEV), V.build_vae_decoder(cfg, seed=11, device=DEV)


def test_instruct_is_its_parts(C, tiny8, vaes):
    from mixdq_amd import Sampler
    enc, dec = vaes
    sm = Sampler(tiny8, "euler", 2, 7.5, image_guidance_scale=1.5)
    _, noise, ehs, added, _, _, _ = _inputs(1, 3, 91, 2, False, C)
    g = torch.Generator(device="cpu").manual_seed(92)
    S = 8 * L_TINY
    pixels = torch.randint(0, 256, (1, 3, S, S), generator=g, dtype=torch.uint8).to(DEV)
    for scale in (1.0, 0.13025):
        moments = enc.moments(pixels)
        cond = C.ip2p_cond(moments, 3, scale)
        if scale == 1.0:
            _same(cond[:1, :4], moments[:, :4], "the unscaled mode of the posterior")
        assert not bool(cond[2:].any())
        want = sm.sample(noise, ehs, added, cond=cond)
        latents, image = sm.instruct(enc, dec, pixels, noise, ehs, added, cond_scale=scale)
        _same(latents, want, f"latents, cond_scale {scale}")
        assert image.dtype == torch.float16 and tuple(image.shape) == (1, 3, S, S)
        _same(image, dec.decode(want), "image")
    by_seed, _ = sm.instruct(enc, dec, pixels, tuple(noise.shape), ehs, added, seed=5)
    _same(by_seed, sm.sample(tuple(noise.shape), ehs, added, seed=5, cond=C.ip2p_cond(enc.moments(pixels), 3)), "seed")
    # refusals: a 4-channel UNet, a two-row Sampler, and inpainting on an 8-channel UNet
    import bench
    from mixdq_amd.unet import SDXLUNet
    with torch.device("meta"):
        unet4 = SDXLUNet(dict(bench.TINY_CFG))
    with pytest.raises(RuntimeError, match="conditioning channels are not the VAE's"):
        Sampler(unet4, "euler", 2, 7.5, image_guidance_scale=1.5).instruct(enc, dec, pixels, noise, ehs, added)
    with pytest.raises(RuntimeError, match="two-row run"):
        Sampler(tiny8, "euler", 2, 7.5).instruct(enc, dec, pixels, noise, ehs, added)
    mask = torch.zeros((1, S, S), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="are not a mask and the VAE's"):
        sm.inpaint_ext(enc, dec, pixels, mask, noise, ehs, added)
