"""Inpainting on the GPU.  mixdq_sampler_step_masked against the numpy restatements (tests/sampler_ref.py's step, then
tests/inpaint_ref.py's blend) bit for bit; mixdq_mask_to_latent against the restatement over dtypes, modes and layouts;
mixdq_composite_u8 against vae.to_uint8 on every FP16 bit pattern and against torch.where; Sampler.sample(mask=) against
an eager loop -- a UNet call, the step, the blend, the FP16 input recomputed -- bit for bit on the tiny UNet of
tests/test_img2img_gpu.py, interleaved with plain and image-to-image calls on one Sampler; and Sampler.inpaint against
its parts done by hand."""
import numpy as np
import pytest
import torch

from tests import inpaint_ref as I
from tests import sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_TINY = 32
f32 = np.float32


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.detach().cpu().contiguous().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {g.size} elements differ"


def _up(v, m):
    return (v + m - 1) // m * m


# ---- the masked step kernel ------------------------------------------------------------------------------------
def _run_masked_steps(C, s, n, channels, rows, with_noise, g, seed, soft=False, start=0):
    """Launch the masked step for every step from `start` on freshly drawn eps and check each launch: the FP32 state,
    every written FP16 input row, the untouched padding behind the n elements (row blocks and noise blocks sit at
    padded strides), the step index and the timestep.  With a binary mask also: kept elements are k, repainted ones
    what the plain step stores."""
    rng = np.random.default_rng(seed)
    coef, t_table, blend = s.coef, s.t_table, s.blend
    n_steps = coef.shape[0]
    rs, ns = _up(n, 8) + 8, _up(n, 4) + 4
    x = (rng.standard_normal(n) * 3).astype(f32)
    z = (rng.standard_normal(n) * 0.2).astype(f32)
    n0 = rng.standard_normal(n).astype(f32)
    mask = rng.random(n // channels).astype(f32) if soft else (rng.random(n // channels) < 0.5).astype(f32)
    m_el = np.repeat(mask, channels)
    noise = rng.standard_normal((n_steps, ns)).astype(f32) if with_noise else None
    x_d, z_d, n0_d, mask_d = t(x), t(z), t(n0), t(mask)
    noise_d = t(noise) if with_noise else None
    coef_d, tt_d, blend_d = t(coef), t(t_table), t(blend)
    step_d = torch.tensor([start], dtype=torch.int32, device=DEV)
    t_d = torch.tensor(-1.0, dtype=torch.float32, device=DEV)
    pad = np.float16(-7.25)
    for i in range(start, n_steps):
        eps = rng.standard_normal((rows, rs)).astype(np.float16)
        eps_d = t(eps)
        inp_d = torch.full((rows, rs), float(pad), dtype=torch.float16, device=DEV)
        # the plain step from the same state, on copies
        px_d, pstep_d, pt_d = x_d.clone(), step_d.clone(), t_d.clone()
        pin_d = torch.zeros((rows, rs), dtype=torch.float16, device=DEV)
        C.sampler_step(px_d, eps_d, pin_d, coef_d, tt_d, pstep_d, pt_d, g, rows, noise_d, n=n, row_stride=rs,
                       noise_stride=ns)
        C.sampler_step_masked(x_d, eps_d, inp_d, coef_d, tt_d, step_d, t_d, z_d, n0_d, mask_d, blend_d, g, rows, noise_d,
                              channels=channels, n=n, row_stride=rs, noise_stride=ns)
        y, _ = R.step(x, eps[0, :n], eps[1, :n] if rows == 2 else None, coef[i], g, noise[i, :n] if with_noise else None)
        _same(px_d, y, f"plain state after step {i}")
        x = I.blend(y, z, n0, m_el, blend[i, 0], blend[i, 1])
        with np.errstate(over="ignore"):
            want_in = (x * f32(coef[i, 3])).astype(np.float16)
        _same(x_d, x, f"state after step {i}")
        got_in = inp_d.cpu().numpy()
        for r in range(rows):
            _same(got_in[r, :n], want_in, f"UNet input row block {r} after step {i}")
        assert (got_in[:, n:] == pad).all(), "the kernel wrote behind its n elements"
        assert int(step_d.item()) == i + 1 and float(t_d.item()) == float(t_table[i + 1])
        if not soft:
            got = x_d.cpu().numpy()
            assert np.array_equal(got[m_el == 0], I.kept(z, n0, blend[i, 0], blend[i, 1])[m_el == 0])
            assert np.array_equal(got[m_el == 1], px_d.cpu().numpy()[m_el == 1])
    # a launch at step index n_steps writes nothing
    before = (x_d.clone(), inp_d.clone())
    C.sampler_step_masked(x_d, eps_d, inp_d, coef_d, tt_d, step_d, t_d, z_d, n0_d, mask_d, blend_d, g, rows, noise_d,
                          channels=channels, n=n, row_stride=rs, noise_stride=ns)
    assert int(step_d.item()) == n_steps and float(t_d.item()) == float(t_table[n_steps])
    assert torch.equal(x_d, before[0]) and torch.equal(inp_d, before[1])


# n: the 8-element body alone, body + tail, the tail alone -- for channels 4 (the two-mask-values-per-pass path) and 3
SHAPES = [(4 * 8 * 8, 4), (4 * 3 * 5, 4), (4, 4), (3 * 7 * 5, 3), (3 * 8 * 8, 3), (6, 3), (8 * 13, 1)]


@pytest.mark.parametrize("n,channels", SHAPES, ids=[f"n{n}c{c}" for n, c in SHAPES])
@pytest.mark.parametrize("with_noise", [False, True], ids=["nonoise", "noise"])
@pytest.mark.parametrize("rows", [1, 2], ids=["rows1", "rows2"])
def test_masked_step_kernel_equals_the_restatement(C, rows, with_noise, n, channels):
    from mixdq_amd.sampler import schedule
    kind = "euler_ancestral" if with_noise else "euler"
    s = schedule(kind, 3)
    g = 7.5 if rows == 2 else 0.0
    _run_masked_steps(C, s, n, channels, rows, with_noise, g, seed=100 * rows + 10 * with_noise + n % 7)
    _run_masked_steps(C, schedule("lcm", 3), n, channels, rows, with_noise, g, seed=7 + n, soft=True)


def test_masked_step_kernel_grid_stride(C):
    """More 8-element vectors than the launch has lanes (the grid is capped at 2048 workgroups of 256): the loop takes
    a second trip; the last two steps of a 4-step table."""
    from mixdq_amd.sampler import schedule
    n = 8 * (2048 * 256 + 37) + 4
    _run_masked_steps(C, schedule("euler", 4), n, 4, 2, False, 5.0, seed=3, start=2)
    _run_masked_steps(C, schedule("euler_ancestral", 4), 3 * (2048 * 256 * 8 // 3 + 50), 3, 1, True, 0.0, seed=4, start=3)


def test_masked_step_refusals(C):
    from mixdq_amd.sampler import schedule
    s = schedule("euler", 2)
    n = 64
    x_d, z_d, n0_d = (torch.zeros(n, device=DEV) for _ in range(3))
    eps_d = torch.zeros(n, dtype=torch.float16, device=DEV)
    inp_d = torch.full((n,), 3.0, dtype=torch.float16, device=DEV)
    mask_d = torch.ones(n // 4, device=DEV)
    step_d = torch.zeros(1, dtype=torch.int32, device=DEV)
    t_d = torch.tensor(5.0, device=DEV)
    args = (x_d, eps_d, inp_d, t(s.coef), t(s.t_table), step_d, t_d, z_d, n0_d, mask_d, t(s.blend))
    with pytest.raises(RuntimeError, match="invalid argument"):
        C.sampler_step_masked(*args, channels=0)
    with pytest.raises(RuntimeError, match="invalid argument"):
        C.sampler_step_masked(*args, channels=3)                  # 64 % 3 != 0
    with pytest.raises(RuntimeError, match="alignment"):
        C.sampler_step_masked(*args[:7], z_d[1:], *args[8:], n=32)
    with pytest.raises(RuntimeError, match="mask should be"):
        C.sampler_step_masked(*args[:9], mask_d[:8], args[10])
    with pytest.raises(RuntimeError, match="blend should be"):
        C.sampler_step_masked(*args[:10], t(s.coef))
    assert int(step_d.item()) == 0 and float(t_d.item()) == 5.0 and bool((inp_d == 3.0).all())     # nothing ran


# ---- mask ingest -----------------------------------------------------------------------------------------------
NP_DT = {"u8": np.uint8, "f16": np.float16, "f32": np.float32}


def _random_mask(rng, shape, dt):
    """About 1 % set (so that ANY is neither all ones nor all zeros), with the threshold's neighbours and, for floats,
    NaN."""
    if dt == "u8":
        vals = np.array([0, 1, 127, 128, 255, 200], dtype=np.uint8)
        p = [0.6, 0.19, 0.2, 0.004, 0.003, 0.003]
    else:
        h = np.float16(0.5)
        vals = np.array([0.0, 0.25, np.nextafter(h, np.float16(0)), h, np.nextafter(h, np.float16(1)), 1.0, np.nan,
                         -1.0], dtype=NP_DT[dt])
        p = [0.5, 0.1, 0.19, 0.004, 0.003, 0.003, 0.1, 0.1]
    return rng.choice(vals, size=shape, p=p)


def _layouts(m):
    """A [B, H, W] numpy mask as GPU tensors of the same values: contiguous, [B, 1, H, W], a transposed view, a strided
    slice, and a contiguous-looking view whose pointer is one element off (no wide loads)."""
    B, H, W = m.shape
    yield "contiguous", t(m)
    yield "b1hw", t(m)[:, None]
    yield "transposed", t(m.transpose(0, 2, 1)).transpose(1, 2)
    big = torch.zeros((B, 2 * H, 3 * W + 1), dtype=t(m).dtype, device=DEV)
    big[:, ::2, 1::3] = t(m)
    yield "slice", big[:, ::2, 1::3]
    flat = torch.zeros(B * H * W + 1, dtype=t(m).dtype, device=DEV)
    flat[1:] = t(m).reshape(-1)
    yield "offset", flat[1:].view(B, H, W)
    rows = torch.zeros((B, H, W + 3), dtype=t(m).dtype, device=DEV)        # unit stride, rows not 8-element aligned
    rows[:, :, :W] = t(m)
    yield "rowpad", rows[:, :, :W]


@pytest.mark.parametrize("hw", [(8, 8), (16, 24), (64, 40)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("dt", ["u8", "f16", "f32"])
def test_mask_to_latent_equals_the_restatement(C, dt, hw):
    H, W = hw
    rng = np.random.default_rng(H * 100 + W + len(dt))
    m = _random_mask(rng, (3, H, W), dt)
    m[0, 0, 0] = m[2, H - 8, W - 8] = 255 if dt == "u8" else 1.0            # NEAREST sees something too
    for mode in ("nearest", "any"):
        want = I.mask_to_latent(m, mode)
        assert want.sum() >= 2 and (want.sum() < want.size or (H, W) == (8, 8))
        for name, view in _layouts(m):
            got = C.mask_to_latent(view, mode)
            assert got.dtype == torch.float32 and tuple(got.shape) == (3, H // 8, W // 8) and got.is_contiguous()
            _same(got, want, f"{dt} {H}x{W} {mode} {name}")
    assert torch.equal(C.mask_to_latent(t(m)), C.mask_to_latent(t(m), "nearest"))        # the default


@pytest.mark.parametrize("dt", ["u8", "f16", "f32"])
def test_mask_threshold_nan_and_the_far_corner(C, dt):
    """The binarisation at its threshold in pixel (0, 0) of successive blocks; and a mask whose only set pixel is the
    last of its 8x8 block: NEAREST does not see it, ANY does."""
    if dt == "u8":
        vals, want = np.array([127, 128, 0, 255], dtype=np.uint8), [0, 1, 0, 1]
    else:
        h = np.float16(0.5)
        vals = np.array([np.nextafter(h, np.float16(0)), h, np.nextafter(h, np.float16(1)), np.nan], dtype=NP_DT[dt])
        want = [0, 1, 1, 0]
    m = np.zeros((1, 8, 32), dtype=NP_DT[dt])
    m[0, 0, ::8] = vals
    for mode in ("nearest", "any"):
        assert C.mask_to_latent(t(m), mode).cpu().reshape(-1).tolist() == want, mode
    m = np.zeros((2, 24, 16), dtype=NP_DT[dt])
    m[1, 8 * 1 + 7, 8 * 1 + 7] = 255 if dt == "u8" else 1.0
    for name, view in _layouts(m):
        assert float(C.mask_to_latent(view, "nearest").sum()) == 0.0, name
        got = C.mask_to_latent(view, "any")
        assert float(got.sum()) == 1.0 and float(got[1, 1, 1]) == 1.0, name


def test_mask_to_latent_refusals_and_empty(C):
    m = torch.zeros((1, 16, 16), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        C.mask_to_latent(m[:, :12])
    with pytest.raises(RuntimeError, match="mode"):
        C.mask_to_latent(m, "bilinear")
    with pytest.raises(RuntimeError, match="mask should be"):
        C.mask_to_latent(m.to(torch.int32))
    with pytest.raises(RuntimeError, match="mask should be"):
        C.mask_to_latent(m[:, None].expand(1, 3, 16, 16))
    assert tuple(C.mask_to_latent(m[:0], "any").shape) == (0, 2, 2)


# ---- pixel composite -------------------------------------------------------------------------------------------
def _decoded_like(values):
    """FP16 [B, 3, H, W] values as VAEDecoder.decode returns them: three channels of a four-channel channels-last
    tensor."""
    B, _, H, W = values.shape
    four = torch.zeros((B, H, W, 4), dtype=torch.float16, device=DEV)
    four[..., :3] = values.permute(0, 2, 3, 1)
    return four.permute(0, 3, 1, 2)[:, :3]


def test_composite_is_to_uint8_on_every_fp16_pattern(C):
    """With the mask all set the launch is vae.to_uint8: all 65 536 FP16 bit patterns (NaNs and infinities included;
    this is what pins mixdq_to_uint8's NaN result), each in every channel."""
    from mixdq_amd import vae as V
    H, W = 128, 256
    pat = (torch.arange(3 * H * W, dtype=torch.int32) % 65536).to(torch.int16).view(torch.float16)
    decoded = _decoded_like(pat.view(1, 3, H, W).to(DEV))
    assert torch.equal(decoded.contiguous().view(torch.int16).cpu().reshape(-1), pat.view(torch.int16))
    original = torch.full((1, 3, H, W), 77, dtype=torch.uint8, device=DEV)
    got = C.composite_u8(decoded, original, torch.full((1, H, W), 255, dtype=torch.uint8, device=DEV))
    want = V.to_uint8(decoded)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 3, H, W) and got.permute(0, 2, 3, 1).is_contiguous()
    diff = got != want
    assert not bool(diff.any()), f"{int(diff.sum())} values differ, first at FP16 bits " \
                                 f"{int(decoded.contiguous().view(torch.int16)[diff][0]) & 0xffff:#06x}"
    # ... and equals the specification's restatement
    _same(got.cpu().numpy(), I.to_uint8(decoded.cpu().numpy()), "composite vs inpaint_ref.to_uint8")
    # with the mask clear it is the original
    got = V.composite_uint8(decoded, original, torch.zeros((1, 1, H, W), dtype=torch.float32, device=DEV))
    assert torch.equal(got, original)


@pytest.mark.parametrize("hw", [(16, 24), (64, 40)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("dt", ["u8", "f16", "f32"])
def test_composite_equals_torch_where(C, dt, hw):
    from mixdq_amd import vae as V
    H, W = hw
    rng = np.random.default_rng(H + W + len(dt))
    g = torch.Generator(device="cpu").manual_seed(H * W)
    values = (torch.randn(2, 3, H, W, generator=g) * 0.8).to(torch.float16).to(DEV)
    m = _random_mask(rng, (2, H, W), dt)
    m[rng.random(m.shape) < 0.4] = 255 if dt == "u8" else 1.0
    set_px = t(I.mask_set(m))[:, None]
    orig_np = rng.integers(0, 256, (2, 3, H, W), dtype=np.uint8)
    originals = {"channels_last": t(orig_np).contiguous(memory_format=torch.channels_last),
                 "slice": None}
    big = torch.zeros((2, 3, H + 2, 2 * W), dtype=torch.uint8, device=DEV)
    big[:, :, 1:H + 1, ::2] = t(orig_np)
    originals["slice"] = big[:, :, 1:H + 1, ::2]
    for dname, decoded in (("decode-like", _decoded_like(values)), ("nchw", values)):
        want = torch.where(set_px, V.to_uint8(decoded), t(orig_np))
        for oname, original in originals.items():
            assert not original.is_contiguous()
            for mname, mask in _layouts(m):
                got = C.composite_u8(decoded, original, mask)
                assert got.permute(0, 2, 3, 1).is_contiguous()
                assert torch.equal(got, want), f"{dt} {H}x{W} {dname} {oname} {mname}"
    with pytest.raises(RuntimeError, match="original should be"):
        C.composite_u8(values, t(orig_np)[:, :, :8], t(m))
    with pytest.raises(RuntimeError, match="mask should have"):
        C.composite_u8(values, t(orig_np), t(m)[:1])
    with pytest.raises(RuntimeError, match="decoded should be"):
        C.composite_u8(values.float(), t(orig_np), t(m))


# ---- the loop --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_unet(C):
    """The tiny W8A8 UNet of tests/test_img2img_gpu.py (latent 32)."""
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


def _inputs(B, rows, seed, n_steps, uses_noise, soft=False):
    from mixdq_amd.quantize_sdxl import example_inputs
    inp = example_inputs(B * rows, L_TINY, DEV, seed=seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    noise = torch.randn(B, 4, L_TINY, L_TINY, generator=g).to(DEV)
    z = (torch.randn(B, 4, L_TINY, L_TINY, generator=g) * 0.13025).to(DEV)        # as VAEEncoder.encode leaves them
    step_noise = torch.randn(n_steps, B, 4, L_TINY, L_TINY, generator=g).to(DEV) if uses_noise else None
    mask = torch.rand(B, L_TINY, L_TINY, generator=g)
    mask = (mask if soft else (mask < 0.5).float()).to(DEV)
    return z, noise, inp["encoder_hidden_states"], inp["added_cond_kwargs"], step_noise, mask


def _eager_inpaint(unet, sampler, z, noise, ehs, added, step_noise, strength, mask):
    """The loop a user would have to write: the start state as the plain / image-to-image run builds it, then per
    step a UNet call, the step's restatement, the blend's restatement, and the FP16 input recomputed from the blend."""
    from mixdq_amd.sampler import img2img_start
    s, rows = sampler.schedule, sampler.rows_per_image
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
    z_np, n0 = z.float().cpu().numpy(), noise.float().cpu().numpy()
    m = np.broadcast_to(mask.cpu().numpy().reshape(B, 1, L_TINY, L_TINY), x.shape)
    for i in range(t0, s.n_steps):
        sample = t(np.concatenate([inp] * rows, axis=0))
        with torch.no_grad():
            eps = unet(sample, torch.tensor(float(s.timesteps[i]), device=DEV), ehs, added)[0]
        eps = eps.float().cpu().numpy().astype(np.float16)
        y, _ = R.step(x, eps[:B], eps[B:] if rows == 2 else None, s.coef[i], sampler.guidance_scale,
                      step_noise[i].float().cpu().numpy() if s.uses_noise else None)
        x = I.blend(y, z_np, n0, m, s.blend[i, 0], s.blend[i, 1])
        with np.errstate(over="ignore"):
            inp = (x * f32(s.coef[i, 3])).astype(np.float16)
    return t0, x


@pytest.mark.parametrize("kind,n_steps,strength,g", [("euler", 4, 0.5, 0.0), ("euler", 4, None, 5.0),
                                                     ("euler_ancestral", 2, 0.5, 0.0), ("lcm", 4, 0.5, 0.0)])
def test_masked_sample_equals_the_eager_loop(tiny_unet, kind, n_steps, strength, g):
    from mixdq_amd import Sampler
    sm = Sampler(tiny_unet, kind, n_steps, guidance_scale=g)
    rows = sm.rows_per_image
    assert rows == (2 if g > 1 else 1)
    for seed, soft in ((71, False), (72, False), (73, True)):       # later runs: other inputs, the same graph
        z, noise, ehs, added, sn, mask = _inputs(2, rows, seed, n_steps, sm.schedule.uses_noise, soft)
        graph = sm._graph_masked
        got = sm.sample(noise, ehs, added, sn, init_latents=z, strength=strength, mask=mask)
        assert sm._graph is None and (graph is None or sm._graph_masked is graph)
        t0, want = _eager_inpaint(tiny_unet, sm, z, noise, ehs, added, sn, strength, mask)
        assert t0 == (0 if strength is None else n_steps // 2) and int(sm._step.item()) == n_steps
        assert got.dtype == torch.float32 and got.shape == noise.shape and bool(torch.isfinite(got).all())
        _same(got, want, f"{kind} x {n_steps} from step {t0}, seed {seed}")
        if not soft:
            # the last blend row is (1, 0): the kept region ends as the image latents themselves
            keep = (mask == 0)[:, None].expand_as(z)
            assert bool(keep.any()) and torch.equal(got[keep], z.float()[keep])
            assert not torch.equal(got[~keep], z.float()[~keep])
    # [B, 1, h, w] is the same mask
    _same(sm.sample(noise, ehs, added, sn, init_latents=z, strength=strength, mask=mask[:, None]), got, "[B, 1, h, w]")


def test_one_sampler_serves_plain_img2img_and_masked_calls(tiny_unet):
    from mixdq_amd import Sampler
    sm = Sampler(tiny_unet, "euler_ancestral", 4)
    z, noise, ehs, added, sn, mask = _inputs(1, 1, 81, 4, True)
    calls = {"plain": lambda s: s.sample(noise, ehs, added, sn),
             "img2img": lambda s: s.sample(noise, ehs, added, sn, init_latents=z, strength=0.5),
             "masked": lambda s: s.sample(noise, ehs, added, sn, init_latents=z, strength=0.5, mask=mask),
             "masked_full": lambda s: s.sample(noise, ehs, added, sn, init_latents=z, mask=mask)}
    first = {k: calls[k](sm) for k in ("plain", "img2img", "masked", "masked_full")}
    graphs = (sm._graph, sm._graph_masked)
    assert graphs[0] is not None and graphs[1] is not None and graphs[0] is not graphs[1]
    for k in ("masked", "plain", "masked_full", "img2img", "plain", "masked"):
        _same(calls[k](sm), first[k], f"{k} after other kinds of call")
    assert (sm._graph, sm._graph_masked) == graphs
    kinds = list(first)
    for i, a in enumerate(kinds):
        for b in kinds[i + 1:]:
            assert not torch.equal(first[a], first[b]), (a, b)
    # a Sampler whose first call is a masked one
    sm2 = Sampler(tiny_unet, "euler_ancestral", 4)
    for k in ("masked", "plain", "img2img", "masked_full"):
        _same(calls[k](sm2), first[k], f"{k} on a Sampler that captured the masked graph first")
    # the refusals leave it usable
    with pytest.raises(RuntimeError, match="mask requires init_latents"):
        sm.sample(noise, ehs, added, sn, mask=mask)
    with pytest.raises(RuntimeError, match="mask requires init_latents"):
        sm.sample(noise, ehs, added, sn, strength=0.5, mask=mask)
    with pytest.raises(RuntimeError, match="mask should be"):
        sm.sample(noise, ehs, added, sn, init_latents=z, strength=0.5, mask=mask[:, :16])
    with pytest.raises(RuntimeError, match="mask should be"):
        sm.sample(noise, ehs, added, sn, init_latents=z, strength=0.5, mask=mask[:, None].expand(1, 4, L_TINY, L_TINY))
    with pytest.raises(RuntimeError, match="mask should be"):
        sm.sample(noise, ehs, added, sn, init_latents=z, strength=0.5, mask=mask.cpu())
    with pytest.raises(RuntimeError, match="mask should be"):
        sm.sample(noise, ehs, added, sn, init_latents=z, strength=0.5, mask=mask.half())
    with pytest.raises(RuntimeError, match="go together"):
        sm.sample(noise, ehs, added, sn, init_latents=z)                          # the old error, word for word
    with pytest.raises(RuntimeError, match=r"init_latents and strength go together \(both, or neither\)"):
        sm.sample(noise, ehs, added, sn, strength=0.5)
    for k in ("masked", "plain"):
        _same(calls[k](sm), first[k], f"{k} after the refusals")


def test_inpaint_is_encode_mask_sample_decode_composite(tiny_unet):
    from mixdq_amd import Sampler, _C
    from mixdq_amd import vae as V
    cfg = dict(V.VAE_SDXL_CONFIG, block_out_channels=(32, 64, 128, 512), layers_per_block=1, norm_num_groups=8)
    enc, dec = V.build_vae_encoder(cfg, seed=11, device=DEV), V.build_vae_decoder(cfg, seed=11, device=DEV)
    sm = Sampler(tiny_unet, "euler", 2)
    _, noise, ehs, added, _, _ = _inputs(1, 1, 91, 2, False)
    g = torch.Generator(device="cpu").manual_seed(92)
    S = 8 * L_TINY
    pixels = torch.randint(0, 256, (1, 3, S, S), generator=g, dtype=torch.uint8).to(DEV)
    latent_noise = torch.randn(1, 4, L_TINY, L_TINY, generator=g).to(DEV)
    mask = torch.zeros((1, S, S), dtype=torch.uint8, device=DEV)
    mask[:, 37:150, 60:201] = 255                                # edges inside 8x8 blocks: the two modes differ
    for ln, strength, mode in ((None, 0.5, "nearest"), (latent_noise, None, "any")):
        latents, image = sm.inpaint(enc, dec, pixels, mask, noise, ehs, added, strength=strength, latent_noise=ln,
                                    mask_mode=mode)
        m = _C.mask_to_latent(mask, mode)
        want = sm.sample(noise, ehs, added, init_latents=enc.encode(pixels, ln), strength=strength, mask=m)
        assert latents.dtype == torch.float32 and torch.equal(latents.view(torch.int32), want.view(torch.int32))
        assert image.dtype == torch.float16 and tuple(image.shape) == (1, 3, S, S)
        assert torch.equal(image.contiguous().view(torch.int16), dec.decode(want).contiguous().view(torch.int16))
        latents2, comp = sm.inpaint(enc, dec, pixels, mask, noise, ehs, added, strength=strength, latent_noise=ln,
                                    mask_mode=mode, composite=True)
        assert torch.equal(latents2.view(torch.int32), want.view(torch.int32))
        assert comp.dtype == torch.uint8 and tuple(comp.shape) == (1, 3, S, S)
        inside = (mask >= 128)[:, None].expand_as(comp)
        assert torch.equal(comp[~inside], pixels[~inside])                       # every other pixel: bit-identical
        assert torch.equal(comp[inside], V.to_uint8(dec.decode(latents2))[inside])
    assert float(_C.mask_to_latent(mask, "any").sum()) > float(_C.mask_to_latent(mask, "nearest").sum())
    with pytest.raises(RuntimeError, match="image should be uint8"):
        sm.inpaint(enc, dec, V.from_uint8(pixels), mask, noise, ehs, added, composite=True)
