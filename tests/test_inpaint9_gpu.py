"""The 9-channel inpainting checkpoints on the GPU.  The three new launches bit for bit against their numpy restatements
(tests/inpaint9_ref.py) over dtypes, layouts and sizes; the split conv_in bit-equal to its two launches as a torch half
add and within its three-rounding bound of the float64 sums; Sampler.sample(cond=) bit-equal to an eager loop that calls
the UNet with cond_term, interleaved over kinds of call on one Sampler, and after a weight reload; Sampler.inpaint on a
9-channel UNet (blend off and on, composite, crop, mask_grow) against its parts done by hand."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import inpaint9_ref as R9
from tests import inpaint_ref as I
from tests import multistep_ref as M
from tests import sampler_ref as R
from tests.test_inpaint9_host import RADII, SIZES, dilate_cases
from tests.test_inpaint_gpu import NP_DT, _layouts, _random_mask

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


# ---- kernel 1: the ingest with the masked pixels blanked -------------------------------------------------------
def _image(rng, shape, dt):
    if dt == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    img = (rng.standard_normal(shape) * 0.8).astype(NP_DT[dt])
    flat = img.reshape(-1)
    flat[::11] = -np.abs(flat[::11])                   # negative sources: -0.0 in the product form, +0.0 here
    flat[5::97] = np.inf
    flat[7::89] = np.nan
    return img


def _image_layouts(img):
    """A [B, C, H, W] numpy image as GPU tensors of the same values: NCHW, channels-last, a strided slice."""
    B, C, H, W = img.shape
    yield "nchw", t(img)
    yield "channels_last", t(img).contiguous(memory_format=torch.channels_last)
    big = torch.zeros((B, C + 1, H + 3, 2 * W + 1), dtype=t(img).dtype, device=DEV)
    big[:, 1:, 2:H + 2, 1::2] = t(img)
    yield "slice", big[:, 1:, 2:H + 2, 1::2]


@pytest.mark.parametrize("hw", [(8, 8), (16, 24), (64, 40)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("dt", ["u8", "f16", "f32"])
def test_blanked_ingest_equals_the_restatement(C, dt, hw):
    H, W = hw
    rng = np.random.default_rng(H * 10 + W + len(dt))
    for ch in (1, 3, 4):
        img = _image(rng, (2, ch, H, W), dt)
        views = list(_image_layouts(img))
        for mdt in ("u8", "f16", "f32"):
            m = _random_mask(rng, (2, H, W), mdt)
            m[rng.random(m.shape) < 0.4] = 255 if mdt == "u8" else 1.0
            want = R9.ingest_masked(img, m)
            assert I.mask_set(m).any() and not I.mask_set(m).all()
            masks = list(_layouts(m))
            # every image layout under the contiguous mask, every mask layout under the NCHW image
            for (iname, iv), (mname, mv) in [(v, masks[0]) for v in views] + [(views[0], mk) for mk in masks[1:]]:
                got = C.image_to_nhwc8_f16(iv, mv)
                assert got.dtype == torch.float16 and tuple(got.shape) == (2, 8, H, W)
                assert got.permute(0, 2, 3, 1).is_contiguous()
                _same(got.permute(0, 2, 3, 1), want, f"{dt} C={ch} {H}x{W} {iname} mask {mdt} {mname}")
        clear = torch.zeros((2, H, W), dtype=torch.uint8, device=DEV)
        for iname, iv in views:
            _same(C.image_to_nhwc8_f16(iv, clear), C.image_to_nhwc8_f16(iv), f"all-clear mask, {iname}")
        full = torch.full((2, 1, H, W), 0.5, dtype=torch.float16, device=DEV)
        assert not _bits(C.image_to_nhwc8_f16(views[0][1], full)).any(), "an all-set mask: every byte zero"


def test_blanked_ingest_refusals_and_empty(C):
    img = torch.zeros((2, 3, 16, 16), dtype=torch.uint8, device=DEV)
    m = torch.zeros((2, 16, 16), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="mask should have"):
        C.image_to_nhwc8_f16(img, m[:1])
    with pytest.raises(RuntimeError, match="mask should have"):
        C.image_to_nhwc8_f16(img, m[:, :8])
    with pytest.raises(RuntimeError, match="mask should be"):
        C.image_to_nhwc8_f16(img, m.cpu())
    with pytest.raises(RuntimeError, match="mask should be"):
        C.image_to_nhwc8_f16(img, m.to(torch.int32))
    with pytest.raises(RuntimeError, match="mask should be"):
        C.image_to_nhwc8_f16(img, m[:, None].expand(2, 3, 16, 16))
    with pytest.raises(RuntimeError, match="1 to 8 channels"):
        C.image_to_nhwc8_f16(torch.zeros((2, 9, 16, 16), dtype=torch.uint8, device=DEV), m)
    assert tuple(C.image_to_nhwc8_f16(img[:0], m[:0]).shape) == (0, 8, 16, 16)


# ---- kernel 2: the conditioning channels -------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (32, 32)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("L", [1, 4, 7])
def test_inpaint_cond_equals_the_restatement(C, L, hw):
    h, w = hw
    rng = np.random.default_rng(L * 100 + h)
    m = rng.random((3, h, w), dtype=np.float32)                                   # a soft mask: the values pass through
    m.reshape(-1)[::3] = rng.choice(np.array([0.0, 1.0], dtype=np.float32), size=m.reshape(-1)[::3].shape)
    z = (rng.standard_normal((3, h, w, L)) * 3).astype(np.float32)
    z.reshape(-1)[::13] = 7e4                                                     # beyond FP16: rounds to inf
    want = R9.inpaint_cond(m, z)
    got = C.inpaint_cond(t(m), t(z).permute(0, 3, 1, 2))
    assert got.dtype == torch.float16 and tuple(got.shape) == (3, 8, h, w) and got.permute(0, 2, 3, 1).is_contiguous()
    _same(got.permute(0, 2, 3, 1), want, f"L={L} {h}x{w}")
    assert not _bits(got[:, L + 1:]).any(), "channels above L are zero"
    _same(C.inpaint_cond(t(m)[:, None], t(z).permute(0, 3, 1, 2)).permute(0, 2, 3, 1), want, "[B, 1, h, w] mask")
    # latents whose storage is only 4-byte aligned (no 16-byte loads)
    flat = torch.zeros(z.size + 1, dtype=torch.float32, device=DEV)
    flat[1:] = t(z).reshape(-1)
    off = flat[1:].view(3, h, w, L).permute(0, 3, 1, 2)
    assert off.data_ptr() % 16 == 4
    _same(C.inpaint_cond(t(m), off).permute(0, 2, 3, 1), want, "latents at a 4-byte offset")


def test_inpaint_cond_refusals_and_empty(C):
    m = torch.zeros((2, 4, 4), dtype=torch.float32, device=DEV)
    z = lambda L: torch.zeros((2, 4, 4, L), dtype=torch.float32, device=DEV).permute(0, 3, 1, 2)   # noqa: E731
    with pytest.raises(RuntimeError, match="1 to 7 channels"):
        C.inpaint_cond(m, z(8))
    with pytest.raises(RuntimeError, match="zl should be"):
        C.inpaint_cond(m, torch.zeros((2, 4, 4, 4), dtype=torch.float32, device=DEV))    # NCHW storage
    with pytest.raises(RuntimeError, match="zl should be"):
        C.inpaint_cond(m, z(4).half())
    with pytest.raises(RuntimeError, match="mask_lat should be"):
        C.inpaint_cond(m[:1], z(4))
    with pytest.raises(RuntimeError, match="mask_lat should be"):
        C.inpaint_cond(m.half(), z(4))
    assert tuple(C.inpaint_cond(m[:0], z(4)[:0]).shape) == (0, 8, 4, 4)


# ---- kernel 3: the mask growth -----------------------------------------------------------------------------------
def _max_pool(binar_u8, r):
    x = (t(binar_u8) >= 128).float()[:, None]
    return (F.max_pool2d(x, 2 * r + 1, 1, r)[:, 0] * 255).to(torch.uint8)


@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_mask_dilate_equals_the_restatement_on_the_host_cases(C, hw):
    H, W = hw
    for name, m in dilate_cases(H, W).items():
        for r in RADII:
            got = C.mask_dilate(t(m), r)
            assert got.dtype == torch.uint8 and tuple(got.shape) == m.shape and got.is_contiguous()
            _same(got, R9.mask_dilate(m, r), f"{name} {H}x{W} r={r}")
            assert torch.equal(got, _max_pool(m, r)), f"{name} {H}x{W} r={r}: max_pool2d"
            if name == "only_image0":
                assert bool(got[0].any()) and not bool(got[1].any()), "nothing leaks into the next image"


@pytest.mark.parametrize("dt", ["u8", "f16", "f32"])
def test_mask_dilate_layouts_dtypes_and_large_radii(C, dt):
    H, W = 64, 40
    rng = np.random.default_rng(len(dt) + 40)
    m = _random_mask(rng, (3, H, W), dt)                                          # about 1 % set, with NaN and the threshold
    m[1] = 0
    m[0, H - 1, 3] = m[2, 0, W - 1] = 255 if dt == "u8" else 1.0
    binar = np.where(I.mask_set(m), np.uint8(255), np.uint8(0))
    for r in (7, 8, 9, 33, W, H, 255):                                            # r >= W, r >= H: whole rows / images
        want = R9.mask_dilate(m, r)
        assert want[0].any() and not want[1].any()
        assert torch.equal(t(want), _max_pool(binar, r)), f"r={r}: restatement vs max_pool2d"
        for name, view in _layouts(m):
            got = C.mask_dilate(view, r)
            assert tuple(got.shape) == tuple(view.shape) and got.is_contiguous()
            _same(got.reshape(3, H, W), want, f"{dt} r={r} {name}")
    assert bool((C.mask_dilate(t(m), 255)[0] == 255).all())
    _same(C.mask_dilate(t(m), 0), binar, "r = 0 is the binarisation")


def test_mask_dilate_refusals_and_empty(C):
    m = torch.zeros((1, 16, 16), dtype=torch.uint8, device=DEV)
    for bad in (256, -1, 1.0, True):
        with pytest.raises(RuntimeError, match="radius should be"):
            C.mask_dilate(m, bad)
    with pytest.raises(RuntimeError, match="mask should be"):
        C.mask_dilate(m.to(torch.int32), 1)
    assert tuple(C.mask_dilate(m[:0], 3).shape) == (0, 16, 16)


# ---- the UNet ----------------------------------------------------------------------------------------------------
def _tiny(in_channels):
    import bench
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet, quantizable_layers
    unet = build_unet(DEV, cfg=dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64,
                                    in_channels=in_channels))
    inputs = example_inputs(2, L_TINY, DEV, in_channels=in_channels, seed=7)
    ckpt = calibrate(unet, [inputs])
    bos_dict = precompute_bos(unet, inputs["encoder_hidden_states"])
    names = list(quantizable_layers(unet))
    # conv_in is IN the activation config: a 9-channel one falls back to FP16 by itself (in_channels % 4 != 0)
    act = {n: 8 for n in names if n != "conv_out" and (in_channels == 9 or n != "conv_in")}
    quantize_unet(unet, bench.Cfg({n: 8 for n in names}, act), ckpt, bos=True, bos_dict=bos_dict)
    unet.set_fused(True)
    return unet


@pytest.fixture(scope="module")
def tiny9(C):
    """The tiny W8A8 UNet of tests/test_inpaint_gpu.py with a 9-channel conv_in (latent 32)."""
    unet = _tiny(9)
    assert unet.cond_channels == 5 and not unet.conv_in.valid_for_acceleration
    assert unet.conv_in._get_name() == "QuantizedConv2dFPFallback" and unet.conv_in.weight.dtype == torch.float16
    yield unet
    del unet
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def tiny4(C):
    unet = _tiny(4)
    assert unet.cond_channels == 0
    yield unet
    del unet
    torch.cuda.empty_cache()


def _cond(B, seed, C):
    """A conditioning tensor as inpaint() builds it: a binary latent mask and latents through mixdq_inpaint_cond_f16."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    m = (torch.rand(B, L_TINY, L_TINY, generator=g) < 0.4).float().to(DEV)
    z = (torch.randn(B, L_TINY, L_TINY, 4, generator=g) * 0.9).to(DEV).permute(0, 3, 1, 2)
    return C.inpaint_cond(m, z)


def test_split_conv_in_is_two_launches_and_within_three_roundings(C, tiny9):
    unet = tiny9
    g = torch.Generator(device="cpu").manual_seed(3)
    x4 = torch.randn(2, 4, L_TINY, L_TINY, generator=g).to(torch.float16).to(DEV)
    cond = _cond(2, 4, C)
    term = unet.cond_term(cond)
    assert term.dtype == torch.float16 and tuple(term.shape) == (2, 64, L_TINY, L_TINY)
    assert term.is_contiguous(memory_format=torch.channels_last)
    _same(unet.cond_term(cond[:, :5]), term, "5 channels == the padded 8")
    junk = cond.clone()
    junk[:, 5:] = 1234.0
    _same(unet.cond_term(junk), term, "the padding's content is irrelevant")
    wx, wc = unet._conv_in_split(refresh=False)
    w = unet.conv_in.weight
    assert torch.equal(wx[:, :4], w[:, :4]) and not bool(wx[:, 4:].any())
    assert torch.equal(wc[:, :5], w[:, 4:]) and not bool(wc[:, 5:].any())
    y = unet._conv_in_with_term(x4, term)
    x8 = torch.zeros((2, 8, L_TINY, L_TINY), dtype=torch.float16, device=DEV).contiguous(
        memory_format=torch.channels_last)
    x8[:, :4] = x4
    _same(y, C.conv2d_f16(x8, wx, None, 1, 1) + term, "the residual epilogue == a torch half add of the two launches")
    # ... and it is what forward(x4, cond_term=) feeds the first block
    from mixdq_amd.quantize_sdxl import example_inputs
    inp = example_inputs(2, L_TINY, DEV, in_channels=9, seed=8)
    seen = []
    hook = unet.down_blocks[0].register_forward_pre_hook(lambda mod, a: seen.append(a[0].detach().clone()))
    try:
        with torch.no_grad():
            out_split = unet(x4, inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"], cond_term=term)[0]
            out_cat = unet(torch.cat([x4, cond[:, :5]], dim=1), inp["timestep"], inp["encoder_hidden_states"],
                           inp["added_cond_kwargs"])[0]
    finally:
        hook.remove()
    _same(seen[0], y, "forward(cond_term=) runs the split conv_in")
    assert bool(torch.isfinite(out_split).all()) and bool(torch.isfinite(out_cat).all())
    d_in = (seen[0].float() - seen[1].float()).abs().max().item()
    d_out = (out_split.float() - out_cat.float()).abs()
    print(f"split vs concatenated: conv_in max |d| {d_in:.3e}; UNet output max |d| {d_out.max().item():.3e}, mean |d| "
          f"{d_out.mean().item():.3e}, output rms {out_cat.float().pow(2).mean().sqrt().item():.3e}")
    # three FP16 roundings (Sx, Sc + b, their sum), the subnormal floor, FP32 accumulation of at most 144 terms
    sx, sc, b, a = R9.split_conv_in_f64(x4.cpu().numpy(), cond[:, :5].cpu().numpy(), w.cpu().numpy(),
                                        unet.conv_in.bias.cpu().numpy())
    yn = y.float().cpu().numpy().astype(np.float64)
    err = np.abs(yn - (sx + sc + b))
    bound = 2.0 ** -11 * (np.abs(sx) + np.abs(sc + b) + np.abs(yn)) + 3 * 2.0 ** -25 + 2.0 ** -16 * a
    print(f"split conv_in vs float64: worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), f"{int((err > bound).sum())} elements outside the three-rounding bound"


def test_forward_refusals_on_the_gpu(C, tiny9, tiny4):
    from mixdq_amd.quantize_sdxl import example_inputs
    inp = example_inputs(2, L_TINY, DEV, in_channels=9, seed=8)
    rest = (inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"])
    x4 = torch.zeros(2, 4, L_TINY, L_TINY, dtype=torch.float16, device=DEV)
    term = tiny9.cond_term(_cond(2, 4, C))
    with pytest.raises(RuntimeError, match="needs cond_term"):
        tiny9(x4, *rest)
    with pytest.raises(RuntimeError, match="cond_term should be"):
        tiny9(x4, *rest, cond_term=term[:1])
    with pytest.raises(RuntimeError, match="cond_term should be"):
        tiny9(x4, *rest, cond_term=term.float())
    with pytest.raises(RuntimeError, match="cond_term should be"):
        tiny9(x4, *rest, cond_term=term.contiguous())                    # NCHW storage
    with pytest.raises(RuntimeError, match="cond should be"):
        tiny9.cond_term(_cond(2, 4, C).float())
    with pytest.raises(RuntimeError, match="cond should be"):
        tiny9.cond_term(_cond(2, 4, C).cpu())
    with pytest.raises(RuntimeError, match="no conditioning channels"):
        tiny4.cond_term(_cond(2, 4, C))
    with pytest.raises(RuntimeError, match="no conditioning channels"):
        tiny4(x4, *rest, cond_term=term)


# ---- the loop ----------------------------------------------------------------------------------------------------
def _inputs(B, rows, seed, n_steps, uses_noise, C):
    from mixdq_amd.quantize_sdxl import example_inputs
    inp = example_inputs(B * rows, L_TINY, DEV, seed=seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    noise = torch.randn(B, 4, L_TINY, L_TINY, generator=g).to(DEV)
    z = (torch.randn(B, 4, L_TINY, L_TINY, generator=g) * 0.13025).to(DEV)
    step_noise = torch.randn(n_steps, B, 4, L_TINY, L_TINY, generator=g).to(DEV) if uses_noise else None
    mask = (torch.rand(B, L_TINY, L_TINY, generator=g) < 0.5).float().to(DEV)
    return z, noise, inp["encoder_hidden_states"], inp["added_cond_kwargs"], step_noise, mask, _cond(B, seed + 2, C)


def _eager(unet, sampler, noise, ehs, added, cond, step_noise=None, z=None, strength=None, mask=None):
    """The loop a user would have to write: unet.cond_term once, then per step a UNet call with cond_term=, the step's
    restatement (order 2: with the history), the blend's where there is a mask, and the FP16 input recomputed."""
    from mixdq_amd.sampler import img2img_start
    s, rows, g = sampler.schedule, sampler.rows_per_image, sampler.guidance_scale
    B = noise.shape[0]
    term = unet.cond_term(cond)
    if term.shape[0] != B * rows:
        term = torch.cat([term] * rows, dim=0).contiguous(memory_format=torch.channels_last)
    if strength is None:
        t0 = 0
        x, inp = R.init(noise.float().cpu().numpy(), s.init_scale, s.input_scale0)
    else:
        t0 = img2img_start(s.n_steps, strength)
        a0, c0, s0 = (torch.tensor(v, dtype=torch.float32, device=DEV) for v in s.start(t0))
        az = z.float() * a0
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
            eps = unet(sample, torch.tensor(float(s.timesteps[i]), device=DEV), ehs, added, cond_term=term)[0]
        eps = eps.float().cpu().numpy().astype(np.float16)
        eu, ec = eps[:B], (eps[B:] if rows == 2 else None)
        if s.order == 2:
            y, hist = M.step(x, hist, eu, ec, s.coef[i], g, M.is_second(s.coef[i], i, t0))
            s_next = s.coef[i, 6]
        else:
            y, _ = R.step(x, eu, ec, s.coef[i], g, step_noise[i].float().cpu().numpy() if s.uses_noise else None)
            s_next = s.coef[i, 3]
        x = y if mask is None else I.blend(y, z_np, n0, m, s.blend[i, 0], s.blend[i, 1])
        inp = M.scaled_input(x, s_next)
    return x


CALLS = {"euler": ("euler", 3, 0.0, {}), "euler_guided": ("euler", 3, 5.0, {}),
         "ancestral": ("euler_ancestral", 3, 0.0, {}), "ancestral_seed": ("euler_ancestral", 3, 0.0, {"seed": 11}),
         "dpmpp_2m": ("dpmpp_2m", 4, 0.0, {}), "masked": ("euler", 3, 0.0, {"mask": True}),
         "img2img": ("euler", 4, 0.0, {"strength": 0.5})}


@pytest.mark.parametrize("call", list(CALLS))
def test_sample_with_cond_equals_the_eager_loop(C, tiny9, call):
    from mixdq_amd import Sampler
    kind, n_steps, g, extra = CALLS[call]
    sm = Sampler(tiny9, kind, n_steps, guidance_scale=g)
    rows = sm.rows_per_image
    graphs, results = None, []
    for seed in (51, 52, 53):                                      # three different cond on one Sampler
        z, noise, ehs, added, sn, mask, cond = _inputs(2, rows, seed, n_steps, sm.schedule.uses_noise, C)
        kw = {}
        if "mask" in extra:
            kw.update(init_latents=z, mask=mask)
        if "strength" in extra:
            kw.update(init_latents=z, strength=extra["strength"])
        if "seed" in extra:
            shape = tuple(noise.shape)
            sd = torch.tensor([extra["seed"], extra["seed"] + 1], dtype=torch.int64, device=DEV)
            got = sm.sample(shape, ehs, added, seed=extra["seed"], cond=cond, **kw)
            noise = C.randn(shape, sd)
            sn = torch.stack([C.randn(shape, sd, C.RNG_STREAM_STEP, i) for i in range(n_steps)])
        else:
            got = sm.sample(noise, ehs, added, sn, cond=cond, **kw)
        now = (sm._graph, sm._graph_masked, sm._graph_rng, sm._graph_masked_rng)
        assert sum(gr is not None for gr in now) == 1 and (graphs is None or now == graphs), "one graph, never re-captured"
        graphs = now
        want = _eager(tiny9, sm, noise, ehs, added, cond, sn, kw.get("init_latents"), kw.get("strength"), kw.get("mask"))
        assert got.dtype == torch.float32 and got.shape == noise.shape and bool(torch.isfinite(got).all())
        _same(got, want, f"{call}, inputs {seed}")
        results.append(got)
    assert not torch.equal(results[0], results[1]) and not torch.equal(results[1], results[2])
    if "seed" not in extra:
        # B rows serve every row block; the 5-channel form is the padded one
        again = sm.sample(noise, ehs, added, sn, cond=torch.cat([cond] * rows, dim=0), **kw)
        _same(again, results[2], "cond with R rows == B rows repeated")
        _same(sm.sample(noise, ehs, added, sn, cond=cond[:, :5], **kw), results[2], "cond with 5 channels")
        assert (sm._graph, sm._graph_masked, sm._graph_rng, sm._graph_masked_rng) == graphs


def test_cond_is_orthogonal_to_the_kind_of_call_and_refusals(C, tiny9, tiny4):
    from mixdq_amd import Sampler
    sm = Sampler(tiny9, "euler_ancestral", 3)
    z, noise, ehs, added, sn, mask, cond = _inputs(1, 1, 61, 3, True, C)
    calls = {"plain": lambda: sm.sample(noise, ehs, added, sn, cond=cond),
             "img2img": lambda: sm.sample(noise, ehs, added, sn, init_latents=z, strength=0.7, cond=cond),
             "masked": lambda: sm.sample(noise, ehs, added, sn, init_latents=z, mask=mask, cond=cond),
             "seeded": lambda: sm.sample(noise, ehs, added, seed=5, cond=cond)}
    first = {k: f() for k, f in calls.items()}
    graphs = (sm._graph, sm._graph_masked, sm._graph_rng)
    assert all(gr is not None for gr in graphs) and sm._graph_masked_rng is None
    for k in ("masked", "plain", "seeded", "img2img", "plain"):
        _same(calls[k](), first[k], f"{k} after other kinds of call")
    assert (sm._graph, sm._graph_masked, sm._graph_rng) == graphs
    with pytest.raises(RuntimeError, match="cond is required"):
        sm.sample(noise, ehs, added, sn)
    for bad in (cond[:, :4], cond[:, :, :16], cond.float(), cond.cpu(), torch.cat([cond] * 3, dim=0), cond[0]):
        with pytest.raises(RuntimeError, match="cond should be"):
            sm.sample(noise, ehs, added, sn, cond=bad)
    _same(calls["plain"](), first["plain"], "after the refusals")
    sm4 = Sampler(tiny4, "euler", 2)
    with pytest.raises(RuntimeError, match="no conditioning channels"):
        sm4.sample(noise, ehs, added, cond=cond)
    assert bool(torch.isfinite(sm4.sample(noise, ehs, added)).all())


def test_a_reloaded_conv_in_reaches_the_captured_graph(C, tiny9):
    from mixdq_amd import Sampler
    sm = Sampler(tiny9, "euler", 3)
    z, noise, ehs, added, sn, mask, cond = _inputs(2, 1, 71, 3, False, C)
    before = sm.sample(noise, ehs, added, cond=cond)
    graph = sm._graph
    old = tiny9.conv_in.weight.clone()
    g = torch.Generator(device="cpu").manual_seed(72)
    w2 = (torch.randn(old.shape, generator=g) * 0.03).to(torch.float16).to(DEV)
    try:
        with torch.no_grad():
            tiny9.conv_in.weight.copy_(w2)
        got = sm.sample(noise, ehs, added, cond=cond)
        assert sm._graph is graph
        _same(got, _eager(tiny9, sm, noise, ehs, added, cond), "after conv_in.weight.copy_: the captured graph")
        assert not torch.equal(got, before)
    finally:
        with torch.no_grad():
            tiny9.conv_in.weight.copy_(old)
    _same(sm.sample(noise, ehs, added, cond=cond), before, "the old weights again")


# ---- inpaint() ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vaes(C):
    from mixdq_amd import vae as V
    cfg = dict(V.VAE_SDXL_CONFIG, block_out_channels=(32, 64, 128, 512), layers_per_block=1, norm_num_groups=8)
    return V.build_vae_encoder(cfg, seed=11, device=DEV), V.build_vae_decoder(cfg, seed=11, device=DEV)


def _pixels(seed, B=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    S = 8 * L_TINY
    pixels = torch.randint(0, 256, (B, 3, S, S), generator=g, dtype=torch.uint8).to(DEV)
    mask = torch.zeros((B, S, S), dtype=torch.uint8, device=DEV)
    mask[:, 37:150, 60:201] = 255
    return pixels, mask, torch.randn(B, 4, L_TINY, L_TINY, generator=g).to(DEV), \
        torch.randn(B, 4, L_TINY, L_TINY, generator=g).to(DEV)


def test_inpaint_on_a_9_channel_unet_is_its_parts(C, tiny9, vaes):
    from mixdq_amd import Sampler
    from mixdq_amd import vae as V
    enc, dec = vaes
    sm = Sampler(tiny9, "euler", 2)
    _, noise, ehs, added, _, _, _ = _inputs(1, 1, 91, 2, False, C)
    pixels, mask, ln, cn = _pixels(92)
    S = 8 * L_TINY
    for mode, strength, blend, cnoise in (("nearest", None, None, None), ("any", 0.5, None, cn), ("any", None, True, cn),
                                          ("nearest", 0.5, True, None)):
        m = C.mask_to_latent(mask, mode)
        zm = enc.encode(pixels, cnoise, mask=mask)
        _same(zm, enc.encode(torch.where((mask >= 128)[:, None], torch.zeros_like(V.from_uint8(pixels)),
                                         V.from_uint8(pixels)), cnoise), "encode(mask=) == encode of the blanked image")
        cond = C.inpaint_cond(m, zm)
        kw = dict(cond=cond)
        if blend:
            kw.update(init_latents=enc.encode(pixels, ln), mask=m, strength=strength)
        elif strength is not None:
            kw.update(init_latents=enc.encode(pixels, ln), strength=strength)
        want = sm.sample(noise, ehs, added, **kw)
        latents, image = sm.inpaint_ext(enc, dec, pixels, mask, noise, ehs, added, strength=strength, latent_noise=ln,
                                        mask_mode=mode, blend=blend, cond_latent_noise=cnoise)
        _same(latents, want, f"latents: {mode} strength {strength} blend {blend}")
        assert image.dtype == torch.float16 and tuple(image.shape) == (1, 3, S, S)
        _same(image, dec.decode(want), "image")
        latents2, comp = sm.inpaint_ext(enc, dec, pixels, mask, noise, ehs, added, strength=strength, latent_noise=ln,
                                        mask_mode=mode, blend=blend, cond_latent_noise=cnoise, composite=True)
        _same(latents2, want, "latents with composite")
        inside = (mask >= 128)[:, None].expand_as(comp)
        assert comp.dtype == torch.uint8 and torch.equal(comp[~inside], pixels[~inside])
        assert torch.equal(comp[inside], V.to_uint8(dec.decode(want))[inside])
    assert sm._graph is not None and sm._graph_masked is not None
    # latent_seed: stream 3 is the blanked image's posterior noise, stream 2 the init image's
    sd = torch.tensor([7], dtype=torch.int64, device=DEV)
    shape = tuple(noise.shape)
    by_seed, _ = sm.inpaint(enc, dec, pixels, mask, noise, ehs, added, strength=0.5, latent_seed=7)
    by_hand, _ = sm.inpaint_ext(enc, dec, pixels, mask, noise, ehs, added, strength=0.5,
                                latent_noise=C.randn(shape, sd, C.RNG_STREAM_VAE, 0),
                                cond_latent_noise=C.randn(shape, sd, C.RNG_STREAM_COND, 0))
    _same(by_seed, by_hand, "latent_seed")
    assert C.RNG_STREAM_COND == 3


def test_inpaint_mask_grow_and_crop_on_a_9_channel_unet(C, tiny9, vaes):
    from mixdq_amd import Sampler
    from mixdq_amd import image as Im
    enc, dec = vaes
    sm = Sampler(tiny9, "euler", 2)
    _, noise, ehs, added, _, _, _ = _inputs(1, 1, 93, 2, False, C)
    pixels, mask, ln, cn = _pixels(94)
    grown = C.mask_dilate(mask, 6)
    assert int((grown >= 128).sum()) == (113 + 12) * (141 + 12)
    a = sm.inpaint_ext(enc, dec, pixels, mask, noise, ehs, added, mask_grow=6, composite=True, mask_mode="any")
    b = sm.inpaint(enc, dec, pixels, grown, noise, ehs, added, composite=True, mask_mode="any")
    _same(a[0], b[0], "mask_grow=6 == the dilated mask: latents")
    _same(a[1], b[1], "mask_grow=6 == the dilated mask: image")
    outside = (grown < 128)[:, None].expand_as(a[1])
    assert torch.equal(a[1][outside], pixels[outside]) and not torch.equal(a[1][~outside], pixels[~outside])
    c = sm.inpaint(enc, dec, pixels, mask, noise, ehs, added, composite=True, mask_mode="any")
    assert not torch.equal(a[0], c[0])
    with pytest.raises(RuntimeError, match="mask_grow should be"):
        sm.inpaint_ext(enc, dec, pixels, mask, noise, ehs, added, mask_grow=256)
    # crop: a larger image, the window resized to the model size, the grown mask everywhere
    g = torch.Generator(device="cpu").manual_seed(95)
    H0, W0 = 300, 420
    big = torch.randint(0, 256, (1, 3, H0, W0), generator=g, dtype=torch.uint8).to(DEV)
    bmask = torch.zeros((1, H0, W0), dtype=torch.uint8, device=DEV)
    bmask[:, 100:180, 150:260] = 255
    box = (100, 60, 340, 300)
    for grow, blur in ((0, 0.0), (6, 3.0)):
        lat, out = sm.inpaint_ext(enc, dec, big, bmask, noise, ehs, added, composite=True, crop=box, mask_blur=blur,
                                  mask_grow=grow, strength=0.5, latent_noise=ln, cond_latent_noise=cn, resample="bicubic")
        mk = C.mask_dilate(bmask, grow) if grow else bmask
        model_hw = (8 * L_TINY, 8 * L_TINY)
        small = Im.resize(big, model_hw, (box,), "bicubic")
        small_mask = Im.resize(mk[:, None], model_hw, (box,), "bilinear", mask=True)[:, 0]
        m = C.mask_to_latent(small_mask, "nearest")
        cond = C.inpaint_cond(m, enc.encode(small, cn, mask=small_mask))
        want = sm.sample(noise, ehs, added, init_latents=enc.encode(small, ln), strength=0.5, cond=cond)
        _same(lat, want, f"crop latents, grow {grow}")
        soft = blur > 0
        pasted = Im.paste(dec.decode(want), big, Im.blur_mask(mk, blur) if soft else mk, (box,), "bicubic", soft=soft)
        _same(out, pasted, f"crop image, grow {grow} blur {blur}")
        weight = Im.blur_mask(mk, blur) if soft else mk
        untouched = (weight == 0)[:, None].expand_as(out)
        assert torch.equal(out[untouched], big[untouched]) and not torch.equal(out, big)
    auto = sm.inpaint_ext(enc, dec, big, bmask, noise, ehs, added, composite=True, crop="auto", mask_grow=6)
    boxes = tuple(Im.crop_region(bb, (H0, W0), (8 * L_TINY, 8 * L_TINY), 32)
                  for bb in Im.mask_bbox(C.mask_dilate(bmask, 6)))
    hand = sm.inpaint(enc, dec, big, C.mask_dilate(bmask, 6), noise, ehs, added, composite=True, crop=boxes)
    _same(auto[1], hand[1], "crop='auto' takes the grown mask's bounding box")


def test_mask_grow_and_blend_on_a_4_channel_unet(C, tiny4, vaes):
    from mixdq_amd import Sampler
    enc, dec = vaes
    sm = Sampler(tiny4, "euler", 2)
    _, noise, ehs, added, _, _, _ = _inputs(1, 1, 96, 2, False, C)
    pixels, mask, ln, _ = _pixels(97)
    grown = C.mask_dilate(mask, 6)
    a = sm.inpaint_ext(enc, dec, pixels, mask, noise, ehs, added, mask_grow=6, composite=True, strength=0.5)
    b = sm.inpaint(enc, dec, pixels, grown, noise, ehs, added, composite=True, strength=0.5)
    _same(a[0], b[0], "latents")
    _same(a[1], b[1], "image")
    want = sm.sample(noise, ehs, added, init_latents=enc.encode(pixels), strength=0.5, mask=C.mask_to_latent(grown))
    _same(a[0], want, "the blend, as before")
    outside = (grown < 128)[:, None].expand_as(a[1])
    assert torch.equal(a[1][outside], pixels[outside])
    _same(sm.inpaint_ext(enc, dec, pixels, mask, noise, ehs, added, strength=0.5, blend=True)[0],
              sm.inpaint(enc, dec, pixels, mask, noise, ehs, added, strength=0.5)[0], "blend=True is the default here")
    with pytest.raises(RuntimeError, match="blend=False"):
        sm.inpaint_ext(enc, dec, pixels, mask, noise, ehs, added, strength=0.5, blend=False)
