"""The device-side noise on the GPU: the map from words to normals over all 2^24 values of either uniform, _C.randn,
the _rng step launches and Sampler.sample(seed=) -- each bit for bit against the numpy restatement (tests/rng_ref.py)
and against the same launch fed the materialised noise."""
import numpy as np
import pytest
import torch

from tests import inpaint_ref as I
from tests import rng_ref as G
from tests import sampler_ref as R
from tests.test_sampler_gpu import L_TINY, _inputs, tiny  # noqa: F401  (the tiny UNet fixture of the sampler tests)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NUM_CU = 256                                # csrc/common.h kNumCU
SHAPES = {"n120": (4, 5, 6), "n36": (4, 3, 3), "n27": (3, 3, 3)}     # n_image % 8 == 0, % 4 == 0 only, odd


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.detach().cpu().contiguous().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {g.size} elements differ"


def _seeds(vals):
    return torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v for v in vals], dtype=torch.int64, device=DEV)


def _storage(x):
    """A [B, C, H, W] channels-last tensor as its storage: [B, H * W * C]."""
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)


# ---- the map from words to normals, exhaustively -----------------------------------------------------------------------
@pytest.mark.parametrize("which", ["u1", "u2"])
def test_normals_from_bits_over_all_values_of_one_uniform(C, which):
    """All 2^24 values of r0 >> 8 (the radius: log, sqrt) with r1 fixed, and of r1 >> 8 (the angle) with r0 fixed; the
    second pair of each call carries them in the other order of low bits."""
    v = np.arange(1 << 24, dtype=np.uint32)
    sweep = ((v << np.uint32(8)) | (v & np.uint32(0xff))).reshape(-1, 2)        # even values: first pair, odd: second
    fixed = np.array([0x9e3779b9, 0x61c88646] if which == "u1" else [0x00000100, 0xfffffeff], dtype=np.uint32)
    w = np.empty((1 << 23, 4), dtype=np.uint32)
    a, b = (0, 1) if which == "u1" else (1, 0)
    w[:, a], w[:, a + 2] = sweep[:, 0], sweep[:, 1]
    w[:, b], w[:, b + 2] = fixed[0], fixed[1]
    got = C.rng_normals_from_bits(t(w.view(np.int32)))
    # the restatement, each function over the 2^24 swept values once (the fixed word's side: two values)
    want = np.empty(w.shape, dtype=np.float32)
    if which == "u1":
        rad = np.sqrt(np.float32(-2.0) * G.log_u24((sweep >> np.uint32(8)).reshape(-1) + np.uint32(1))).reshape(-1, 2)
        sn, cs = G.sincos_u24(fixed >> np.uint32(8))
    else:
        rad = np.sqrt(np.float32(-2.0) * G.log_u24((fixed >> np.uint32(8)) + np.uint32(1)))
        sn, cs = (f.reshape(-1, 2) for f in G.sincos_u24((sweep >> np.uint32(8)).reshape(-1)))
    want[:, 0::2] = rad * cs
    want[:, 1::2] = rad * sn
    for rows in (slice(0, 1000), slice(-1000, None)):                   # ... which is normals_from_bits, as a whole
        assert np.array_equal(_bits(want[rows]), _bits(G.normals_from_bits(w[rows])))
    assert np.isfinite(want).all()
    _same(got, want, f"normals over all 2^24 values of {which}")


# ---- _C.randn -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream,step", [(0, 0), (1, 5), (2, 0), (3, 0xffffffff)])
@pytest.mark.parametrize("shape", list(SHAPES.values()), ids=list(SHAPES))
def test_randn_equals_the_restatement(C, shape, stream, step):
    seeds = [7, 0x0123456789abcdef, 2 ** 64 - 3]            # a high word; a negative int64
    sd = _seeds(seeds)
    assert sd[2].item() == -3
    got = C.randn((3,) + shape, sd, stream, step)
    assert got.shape == (3,) + shape and got.dtype == torch.float32 and got.permute(0, 2, 3, 1).is_contiguous()
    _same(got, G.randn((3,) + shape, seeds, stream, step), f"randn {shape} stream {stream} step {step}")
    # batch invariance: row b of the batch is the batch-1 call with its seed
    for b in range(3):
        _same(C.randn((1,) + shape, sd[b:b + 1].clone(), stream, step), got[b:b + 1], f"row {b} alone")
    # out=: filled in place, nothing beside it
    n = int(np.prod(shape))
    buf = torch.full((3 * n + 8,), -7.25, device=DEV)
    out = buf[4:4 + 3 * n].view(3, shape[1], shape[2], shape[0]).permute(0, 3, 1, 2)
    assert C.randn((3,) + shape, sd, stream, step, out=out) is out
    _same(out, got, "randn(out=)")
    assert (buf[:4] == -7.25).all() and (buf[4 + 3 * n:] == -7.25).all()


def test_randn_grid_stride(C):
    """More elements than one pass of the capped grid covers, n_image % 4 == 0 and not (the partly used last call far
    into the stride loop)."""
    for n_image, B in ((NUM_CU * 8 * 256 * 8 + 4 * 37, 1), ((NUM_CU * 8 * 256 * 8 + 4 * 37) // 2 + 3, 2)):
        seeds = [0xdeadbeef00000001 + b for b in range(B)]
        got = C.randn((B, 1, 1, n_image), _seeds(seeds))
        _same(got, G.randn((B, 1, 1, n_image), seeds), f"randn n_image {n_image} B {B}")


def test_randn_refusals(C):
    sd = _seeds([1, 2])
    with pytest.raises(RuntimeError, match="seeds"):
        C.randn((3, 4, 2, 2), sd)
    with pytest.raises(RuntimeError, match="out should be"):
        C.randn((2, 4, 2, 2), sd, out=torch.zeros(2, 4, 2, 2, device=DEV))           # NCHW-dense, not channels-last
    with pytest.raises(RuntimeError, match="alignment"):
        buf = torch.zeros(2 * 16 + 4, device=DEV)
        C.randn((2, 4, 2, 2), sd, out=buf[1:33].view(2, 2, 2, 4).permute(0, 3, 1, 2))


# ---- the _rng step launches ---------------------------------------------------------------------------------------------
def _run_rng_steps(C, shape, rows, start, masked, seed):
    from mixdq_amd.sampler import schedule
    s = schedule("euler_ancestral", 4)
    rng = np.random.default_rng(seed)
    B = 3
    Cc, H, W = shape
    n_image = Cc * H * W
    n = B * n_image
    seeds = [seed, 0x8000000000000000 + seed, (seed << 33) + 1]
    sd = _seeds(seeds)
    g = 6.5 if rows == 2 else 0.0
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    rs = (n + 7) // 8 * 8 + 8
    coef_d, tt_d = t(s.coef), t(s.t_table)
    state = {k: dict(x=t(x), step=torch.tensor([start], dtype=torch.int32, device=DEV),
                     ts=torch.tensor(-1.0, device=DEV)) for k in ("rng", "buf")}
    ns = (n + 3) // 4 * 4 + 4                   # the buffer-fed sibling wants its noise blocks a multiple of 4 apart
    noise_d = torch.zeros((4, ns), device=DEV)
    for i in range(4):
        noise_d[i, :n] = _storage(C.randn((B,) + shape, sd, C.RNG_STREAM_STEP, i)).reshape(-1)
    extra, extra_np = {}, None
    if masked:
        z, n0 = rng.standard_normal((2, n)).astype(np.float32)
        m = rng.choice(np.array([0.0, 1.0, 0.25], dtype=np.float32), n // Cc)
        extra = dict(channels=Cc)
        extra_np = (z, n0, np.repeat(m, Cc))
        margs = (t(z), t(n0), t(m), t(s.blend))
    pad = np.float16(-7.25)
    for i in range(start, 4):
        eps = rng.standard_normal((rows, rs)).astype(np.float16)
        inps = {}
        for k in ("rng", "buf"):
            st = state[k]
            inps[k] = torch.full((rows, rs), float(pad), dtype=torch.float16, device=DEV)
            kw = dict(seeds=sd, n_image=n_image) if k == "rng" else dict(noise_stride=ns)
            noise = None if k == "rng" else noise_d
            if masked:
                C.sampler_step_masked(st["x"], t(eps), inps[k], coef_d, tt_d, st["step"], st["ts"], *margs, g, rows,
                                      noise, n=n, row_stride=rs, **extra, **kw)
            else:
                C.sampler_step(st["x"], t(eps), inps[k], coef_d, tt_d, st["step"], st["ts"], g, rows, noise, n=n,
                               row_stride=rs, **kw)
        ref_noise = np.concatenate([G.randn_image(sv, n_image, G.STREAM_STEP, i) for sv in seeds])
        _same(noise_d[i, :n], ref_noise, f"randn(stream 1, step {i})")
        x, want_in = R.step(x, eps[0, :n], eps[1, :n] if rows == 2 else None, s.coef[i], g, ref_noise)
        if masked:
            x = I.blend(x, extra_np[0], extra_np[1], extra_np[2], s.blend[i, 0], s.blend[i, 1])
            with np.errstate(over="ignore"):
                want_in = (x * np.float32(s.coef[i, 3])).astype(np.float16)
        for k in ("rng", "buf"):
            _same(state[k]["x"], x, f"{k}: state after step {i}")
            got_in = inps[k].cpu().numpy()
            for r in range(rows):
                _same(got_in[r, :n], want_in, f"{k}: UNet input row block {r} after step {i}")
            assert (got_in[:, n:] == pad).all(), f"{k}: the kernel wrote behind its n elements"
            assert int(state[k]["step"].item()) == i + 1 and float(state[k]["ts"].item()) == float(s.t_table[i + 1])
    # past the end of the table nothing is written
    st = state["rng"]
    before = st["x"].clone()
    inp = torch.full((rows, rs), float(pad), dtype=torch.float16, device=DEV)
    eps_d = torch.ones((rows, rs), dtype=torch.float16, device=DEV)
    if masked:
        C.sampler_step_masked(st["x"], eps_d, inp, coef_d, tt_d, st["step"], st["ts"], *margs, g, rows, None, n=n,
                              row_stride=rs, seeds=sd, n_image=n_image, **extra)
    else:
        C.sampler_step(st["x"], eps_d, inp, coef_d, tt_d, st["step"], st["ts"], g, rows, None, n=n, row_stride=rs,
                       seeds=sd, n_image=n_image)
    assert torch.equal(st["x"], before) and (inp == float(pad)).all()
    assert int(st["step"].item()) == 4 and float(st["ts"].item()) == float(s.t_table[4])


@pytest.mark.parametrize("start", [0, 2])
@pytest.mark.parametrize("rows", [1, 2], ids=["rows1", "rows2"])
@pytest.mark.parametrize("shape", list(SHAPES.values()), ids=list(SHAPES))
def test_step_rng_equals_the_buffer_fed_step_and_the_restatement(C, shape, rows, start):
    _run_rng_steps(C, shape, rows, start, False, seed=100 + 10 * rows + start)


@pytest.mark.parametrize("start", [0, 2])
@pytest.mark.parametrize("rows", [1, 2], ids=["rows1", "rows2"])
@pytest.mark.parametrize("shape", [(4, 5, 6), (4, 3, 3), (3, 3, 3), (3, 2, 4)], ids=["c4n120", "c4n36", "c3n27", "c3n24"])
def test_step_masked_rng_equals_the_buffer_fed_step_and_the_restatement(C, shape, rows, start):
    _run_rng_steps(C, shape, rows, start, True, seed=200 + 10 * rows + start)


def test_step_rng_more_vectors_than_lanes(C):
    """The stride loop of the step launch with generated noise: more 8-element vectors than the capped grid has lanes,
    one image; checked against the buffer-fed launch (the restatement covers the same values in the randn test)."""
    from mixdq_amd.sampler import schedule
    s = schedule("euler_ancestral", 2)
    n = 8 * (NUM_CU * 8 * 256 + 37)
    sd = _seeds([0xabcdef0123456789])
    g = torch.Generator(device="cpu").manual_seed(3)
    x0 = torch.randn(n, generator=g).to(DEV)
    eps = torch.randn(n, generator=g).to(torch.float16).to(DEV)
    noise = torch.stack([C.randn((1, 1, 1, n), sd, C.RNG_STREAM_STEP, i).reshape(-1) for i in range(2)])
    coef_d, tt_d = t(s.coef), t(s.t_table)
    res = {}
    for k in ("rng", "buf"):
        x, inp = x0.clone(), torch.zeros(n, dtype=torch.float16, device=DEV)
        step, ts = torch.zeros(1, dtype=torch.int32, device=DEV), torch.tensor(0.0, device=DEV)
        kw = dict(seeds=sd) if k == "rng" else {}
        C.sampler_step(x, eps, inp, coef_d, tt_d, step, ts, 0.0, 1, None if k == "rng" else noise, **kw)
        res[k] = (x, inp)
    _same(res["rng"][0], res["buf"][0], "state")
    _same(res["rng"][1], res["buf"][1], "UNet input")
    assert not torch.equal(res["rng"][0], x0)


# ---- Sampler.sample(seed=) ----------------------------------------------------------------------------------------------
def _materialise(C, shape, seeds, n_steps):
    sd = _seeds(seeds)
    return C.randn(shape, sd), torch.stack([C.randn(shape, sd, C.RNG_STREAM_STEP, i) for i in range(n_steps)])


CONFIGS = {"ea": ("euler_ancestral", 0.0, "plain"), "ea_guided": ("euler_ancestral", 7.5, "plain"),
           "lcm": ("lcm", 0.0, "plain"), "ea_img2img": ("euler_ancestral", 0.0, "img2img"),
           "ea_masked": ("euler_ancestral", 0.0, "masked")}


@pytest.mark.parametrize("config", list(CONFIGS))
def test_sampler_seed_equals_the_materialised_run(C, tiny, config):  # noqa: F811
    from mixdq_amd import Sampler
    kind, g, mode = CONFIGS[config]
    n_steps, B = 3, 2
    sm, ref = Sampler(tiny, kind, n_steps, guidance_scale=g), Sampler(tiny, kind, n_steps, guidance_scale=g)
    shape = (B, 4, L_TINY, L_TINY)
    noise_t, ehs, added, sn_t = _inputs(B, sm.rows_per_image, L_TINY, 31, n_steps)
    kw = {}
    if mode != "plain":
        gen = torch.Generator(device="cpu").manual_seed(5)
        kw["init_latents"] = torch.randn(shape, generator=gen).to(DEV)
        if mode == "img2img":
            kw["strength"] = 0.7                                       # 3 steps: the run starts at step 1
            from mixdq_amd.sampler import img2img_start
            assert img2img_start(n_steps, 0.7) == 1
        else:
            kw["mask"] = (torch.rand((B, L_TINY, L_TINY), generator=gen) < 0.5).float().to(DEV)
    graph_name = "_graph_masked_rng" if mode == "masked" else "_graph_rng"
    results = []
    for seed in (11, 0xfedcba9876543210):
        graph = getattr(sm, graph_name)
        got = sm.sample(shape, ehs, added, seed=seed, **kw)
        assert graph is None or getattr(sm, graph_name) is graph              # the second seed: no re-capture
        seeds = [(seed + b) % 2 ** 64 for b in range(B)]
        noise, sn = _materialise(C, shape, seeds, n_steps)
        _same(got, ref.sample(noise, ehs, added, sn, **kw), f"{config}: seed {seed:#x} != its materialised run")
        assert torch.isfinite(got).all()
        results.append(got)
    assert not torch.equal(results[0], results[1])
    assert sm._noise is None and sm._graph is None and sm._graph_masked is None   # seed only: no [n_steps, ...] buffer
    # seeded and unseeded calls alternate; the unseeded results are those of a Sampler that never saw a seed
    plain = ref.sample(noise_t, ehs, added, sn_t, **kw)
    _same(sm.sample(noise_t, ehs, added, sn_t, **kw), plain, f"{config}: unseeded after seeded")
    _same(sm.sample(shape, ehs, added, seed=11, **kw), results[0], f"{config}: seeded after unseeded")
    _same(sm.sample(noise_t, ehs, added, sn_t, **kw), plain, f"{config}: unseeded again")
    # a sequence and a tensor of seeds; with a noise tensor only the step noise comes from the seed
    _same(sm.sample(shape, ehs, added, seed=[11, 12], **kw), results[0], f"{config}: a sequence of seeds")
    _same(sm.sample(shape, ehs, added, seed=_seeds([11, 12]), **kw), results[0], f"{config}: a tensor of seeds")
    _, sn = _materialise(C, shape, [11, 12], n_steps)
    _same(sm.sample(noise_t, ehs, added, seed=11, **kw), ref.sample(noise_t, ehs, added, sn, **kw),
          f"{config}: a noise tensor with seed")
    assert ref._graph_rng is None and ref._graph_masked_rng is None and ref._seeds is None
    with pytest.raises(RuntimeError, match="step_noise must be None"):
        sm.sample(shape, ehs, added, sn_t, seed=11, **kw)


def test_sampler_seed_on_a_kind_without_step_noise(C, tiny):  # noqa: F811
    from mixdq_amd import Sampler
    sm, ref = Sampler(tiny, "dpmpp_2m", 3), Sampler(tiny, "dpmpp_2m", 3)
    shape = (2, 4, L_TINY, L_TINY)
    _, ehs, added, _ = _inputs(2, 1, L_TINY, 41, 3, uses_noise=False)
    got = sm.sample(shape, ehs, added, seed=2 ** 64 - 1)                          # image 1: seed 0 (mod 2^64)
    noise = C.randn(shape, _seeds([2 ** 64 - 1, 0]))
    _same(got, ref.sample(noise, ehs, added), "dpmpp_2m: seed != the run fed that start noise")
    assert sm._graph is not None and sm._graph_rng is None
    _same(sm.sample(noise, ehs, added), got, "dpmpp_2m: unseeded on the same graph")


def test_seed_is_per_image(C, tiny):  # noqa: F811
    """seed=5 at B = 2 starts image 1 from the noise seed=6 gives at B = 1, and adds the same step noise to it: compared
    on the noise itself (the static start buffer, the seed buffer the step launches read, and what those launches
    compute from it -- test_step_rng_* ties that to randn), not on the UNet's output."""
    from mixdq_amd import Sampler
    shape2, shape1 = (2, 4, L_TINY, L_TINY), (1, 4, L_TINY, L_TINY)
    sm2, sm1 = Sampler(tiny, "euler_ancestral", 2), Sampler(tiny, "euler_ancestral", 2)
    _, ehs, added, _ = _inputs(2, 1, L_TINY, 51, 2)
    sm2.sample(shape2, ehs, added, seed=5)
    sm1.sample(shape1, ehs[1:2].contiguous(), {k: v[1:2].contiguous() for k, v in added.items()}, seed=6)
    assert sm2._seeds.tolist() == [5, 6] and sm1._seeds.tolist() == [6]
    _same(sm2._start[1:2], sm1._start, "start noise of image 1")
    _same(sm2._start, G.randn(shape2, [5, 6]), "start noise")
    for i in range(2):
        _same(C.randn(shape2, sm2._seeds, C.RNG_STREAM_STEP, i)[1:2], C.randn(shape1, sm1._seeds, C.RNG_STREAM_STEP, i),
              f"step noise {i} of image 1")


def test_seed_passes_through_sample_image_img2img_and_inpaint(C, tiny):  # noqa: F811
    """seed= reaches sample() through the three wrappers, latent_seed= draws the VAE posterior's noise from stream 2, and
    seed alone leaves the posterior the mode: each call equals the same call fed the materialised tensors."""
    from mixdq_amd import Sampler
    from mixdq_amd import vae as V
    cfg = dict(V.VAE_SDXL_CONFIG, block_out_channels=(32, 64, 128, 512), layers_per_block=1, norm_num_groups=8)
    enc, dec = V.build_vae_encoder(cfg, seed=11, device=DEV), V.build_vae_decoder(cfg, seed=11, device=DEV)
    sm, ref = Sampler(tiny, "euler_ancestral", 3), Sampler(tiny, "euler_ancestral", 3)
    shape = (1, 4, L_TINY, L_TINY)
    _, ehs, added, _ = _inputs(1, 1, L_TINY, 71, 3)
    g = torch.Generator(device="cpu").manual_seed(72)
    pixels = torch.randint(0, 256, (1, 3, 8 * L_TINY, 8 * L_TINY), generator=g, dtype=torch.uint8).to(DEV)
    mask = (torch.rand((1, 8 * L_TINY, 8 * L_TINY), generator=g) < 0.5).to(torch.uint8).mul(255).to(DEV)
    noise, sn = _materialise(C, shape, [9], 3)
    ln = C.randn(shape, _seeds([10]), C.RNG_STREAM_VAE)
    _same(ln, G.randn(shape, [10], G.STREAM_VAE), "the posterior's noise")
    for kw_seed, kw_ref in ((dict(seed=9, latent_seed=10), dict(step_noise=sn, latent_noise=ln)),
                            (dict(seed=9), dict(step_noise=sn))):
        got = sm.img2img(enc, dec, pixels, shape, ehs, added, strength=0.7, **kw_seed)
        want = ref.img2img(enc, dec, pixels, noise, ehs, added, strength=0.7, **kw_ref)
        _same(got[0], want[0], f"img2img latents {sorted(kw_seed)}")
        _same(got[1], want[1], f"img2img image {sorted(kw_seed)}")
        got = sm.inpaint(enc, dec, pixels, mask, shape, ehs, added, **kw_seed)
        want = ref.inpaint(enc, dec, pixels, mask, noise, ehs, added, **kw_ref)
        _same(got[0], want[0], f"inpaint latents {sorted(kw_seed)}")
        _same(got[1], want[1], f"inpaint image {sorted(kw_seed)}")
    got = sm.sample_image(dec, shape, ehs, added, seed=9)
    want = ref.sample_image(dec, noise, ehs, added, sn)
    _same(got[0], want[0], "sample_image latents")
    _same(got[1], want[1], "sample_image image")
    with pytest.raises(RuntimeError, match="exclude each other"):
        sm.img2img(enc, dec, pixels, shape, ehs, added, strength=0.7, seed=9, latent_seed=10, latent_noise=ln)
