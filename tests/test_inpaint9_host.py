"""The 9-channel inpainting checkpoints, host side: the numpy restatements (tests/inpaint9_ref.py) against independent
references -- scipy's and PIL's maximum filters for the mask growth, diffusers' `image * (mask < 0.5)` for the blanked
ingest -- the two new configs, and the split conv_in against the concatenated one on a tiny CPU UNet in float64."""
import numpy as np
import pytest
import torch

from tests import inpaint9_ref as R9
from tests import inpaint_ref as I

RADII = (0, 1, 3, 8, 40)
SIZES = ((16, 24), (13, 40))


def dilate_cases(H, W):
    """name -> uint8 [B, H, W] masks: random (about 3 % set, with the threshold's neighbours), one set pixel in each
    corner, and a batch of two of which only image 0 holds anything."""
    rng = np.random.default_rng(H * 100 + W)
    rand = rng.choice(np.array([0, 127, 128, 255], dtype=np.uint8), size=(2, H, W), p=[0.6, 0.37, 0.015, 0.015])
    cases = {"random": rand}
    for name, (y, x) in (("corner00", (0, 0)), ("corner0W", (0, W - 1)), ("cornerH0", (H - 1, 0)),
                         ("cornerHW", (H - 1, W - 1))):
        m = np.zeros((1, H, W), dtype=np.uint8)
        m[0, y, x] = 200
        cases[name] = m
    only0 = np.zeros((2, H, W), dtype=np.uint8)
    only0[0] = rand[0]
    only0[0, H - 1, W // 2] = 255                       # the last row of image 0 touches the first row of image 1
    cases["only_image0"] = only0
    return cases


@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("r", RADII)
def test_dilate_restatement_is_the_square_maximum_filter(hw, r):
    from PIL import Image, ImageFilter
    from scipy import ndimage
    H, W = hw
    for name, m in dilate_cases(H, W).items():
        got = R9.mask_dilate(m, r)
        assert got.dtype == np.uint8 and got.shape == m.shape and set(np.unique(got)) <= {0, 255}
        binar = np.where(I.mask_set(m), np.uint8(255), np.uint8(0))
        for b in range(m.shape[0]):
            want = ndimage.maximum_filter(binar[b], size=2 * r + 1, mode="constant", cval=0)
            assert np.array_equal(got[b], want), f"{name} image {b} r {r}: scipy"
            pil = np.asarray(Image.fromarray(binar[b]).filter(ImageFilter.MaxFilter(2 * r + 1)))
            assert np.array_equal(got[b], pil), f"{name} image {b} r {r}: PIL"
        if name == "only_image0":
            assert got[0].any() and not got[1].any()
        if name.startswith("corner"):
            assert int((got == 255).sum()) == min(r + 1, H) * min(r + 1, W)
    assert np.array_equal(R9.mask_dilate(m, 0), binar)


@pytest.mark.parametrize("dt", ["u8", "f16", "f32"])
def test_blanked_ingest_restatement_is_image_times_not_mask(dt):
    """from_uint8(image) * (mask < 0.5), diffusers' masked image, up to the sign of zero; float masks with the
    threshold's neighbours."""
    from mixdq_amd import vae as V
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (2, 3, 16, 24), dtype=np.uint8)
    if dt == "u8":
        mask = rng.choice(np.array([0, 127, 128, 255], dtype=np.uint8), size=(2, 16, 24))
        as_float = mask.astype(np.float32) / np.float32(255.0)
    else:
        h = np.float16(0.5)
        vals = np.array([0.0, np.nextafter(h, np.float16(0)), h, np.nextafter(h, np.float16(1)), 1.0],
                        dtype={"f16": np.float16, "f32": np.float32}[dt])
        mask = rng.choice(vals, size=(2, 16, 24))
        as_float = mask.astype(np.float32)
    got = R9.ingest_masked(img, mask)
    keep = torch.from_numpy(as_float < 0.5)[:, None]
    want = (V.from_uint8(torch.from_numpy(img)) * keep).permute(0, 2, 3, 1).numpy()
    assert got.shape == (2, 16, 24, 8) and not got[..., 3:].any()
    assert np.array_equal(got[..., :3], want)                                    # (-0.0 == +0.0)
    blank = I.mask_set(mask)
    assert blank.any() and not blank.all()
    assert not got[blank].view(np.uint16).any(), "a blanked pixel is +0.0 in every channel"
    assert np.array_equal(got[~blank].view(np.uint16), R9.ER.ingest(img)[~blank].view(np.uint16))


def test_inpaint_cond_restatement_layout():
    rng = np.random.default_rng(6)
    m, z = rng.random((2, 5, 7), dtype=np.float32), rng.standard_normal((2, 5, 7, 4)).astype(np.float32)
    out = R9.inpaint_cond(m, z)
    assert np.array_equal(out[..., 0], m.astype(np.float16)) and np.array_equal(out[..., 1:5], z.astype(np.float16))
    assert not out[..., 5:].view(np.uint16).any()


def test_new_entry_points_validate_before_launching():
    """Null pointers, negative sizes, bad dtype codes, out-of-range counts: MIXDQ_ERR_INVALID_ARG (1); misaligned
    pointers: MIXDQ_ERR_ALIGNMENT (2); empty work: MIXDQ_OK with no pointer looked at.  Host code: no GPU needed."""
    import ctypes
    from mixdq_amd.build import build
    lib = ctypes.CDLL(build())
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    ing = lib.mixdq_image_to_nhwc8_f16_masked
    ing.argtypes = [vp, i32] + [i64] * 4 + [vp, i32] + [i64] * 3 + [vp, i32, i32, i32, i32, vp]
    ok = dict(img=0x1000, dt=0, mask=0x2000, mdt=0, out=0x3000, B=1, C=3, H=8, W=8)

    def call_ing(**kw):
        a = dict(ok, **kw)
        return ing(a["img"], a["dt"], 192, 64, 8, 1, a["mask"], a["mdt"], 64, 8, 1, a["out"], a["B"], a["C"], a["H"],
                   a["W"], None)
    for bad in (dict(img=None), dict(mask=None), dict(out=None), dict(B=-1), dict(H=-8), dict(C=0), dict(C=9),
                dict(dt=3), dict(mdt=3), dict(mdt=-1)):
        assert call_ing(**bad) == 1, bad
    for bad in (dict(out=0x3008), dict(img=0x1001, dt=1), dict(img=0x1002, dt=2), dict(mask=0x2001, mdt=1),
                dict(mask=0x2002, mdt=2)):
        assert call_ing(**bad) == 2, bad
    assert call_ing(B=0, img=None, mask=None, out=None) == 0 and call_ing(W=0, img=None, mask=None, out=None) == 0
    cond = lib.mixdq_inpaint_cond_f16
    cond.argtypes = [vp, vp, vp, i64, i32, vp]
    for args in ((None, 0x2000, 0x3000, 4, 4), (0x1000, None, 0x3000, 4, 4), (0x1000, 0x2000, None, 4, 4),
                 (0x1000, 0x2000, 0x3000, -1, 4), (0x1000, 0x2000, 0x3000, 4, 0), (0x1000, 0x2000, 0x3000, 4, 8)):
        assert cond(*args, None) == 1, args
    for args in ((0x1002, 0x2000, 0x3000, 4, 4), (0x1000, 0x2002, 0x3000, 4, 4), (0x1000, 0x2000, 0x3008, 4, 4)):
        assert cond(*args, None) == 2, args
    assert cond(None, None, None, 0, 4, None) == 0
    dil = lib.mixdq_mask_dilate_u8
    dil.argtypes = [vp, i32, i64, i64, i64, vp, vp, i32, i32, i32, i32, vp]
    for args in ((None, 0, 0x2000, 0x3000, 1, 8, 8, 1), (0x1000, 0, None, 0x3000, 1, 8, 8, 1),
                 (0x1000, 0, 0x2000, None, 1, 8, 8, 1), (0x1000, 0, 0x2000, 0x2000, 1, 8, 8, 1),
                 (0x1000, 3, 0x2000, 0x3000, 1, 8, 8, 1), (0x1000, 0, 0x2000, 0x3000, -1, 8, 8, 1),
                 (0x1000, 0, 0x2000, 0x3000, 1, 8, 8, -1), (0x1000, 0, 0x2000, 0x3000, 1, 8, 8, 256)):
        m, dt, scratch, out, B, H, W, r = args
        assert dil(m, dt, 64, 8, 1, scratch, out, B, H, W, r, None) == 1, args
    assert dil(0x1002, 2, 64, 8, 1, 0x2000, 0x3000, 1, 8, 8, 1, None) == 2
    assert dil(None, 0, 64, 8, 1, None, None, 0, 8, 8, 1, None) == 0


def test_inpaint_ext_is_inpaint_plus_three_keywords():
    """Sampler.inpaint keeps its signature; inpaint_ext has the same parameters with the same defaults, then blend,
    mask_grow and cond_latent_noise; the refusals of the new keywords come before anything touches the GPU."""
    import inspect
    from mixdq_amd import sampler as S
    old, ext = inspect.signature(S.Sampler.inpaint).parameters, inspect.signature(S.Sampler.inpaint_ext).parameters
    new = {"blend": None, "mask_grow": 0, "cond_latent_noise": None}
    assert list(ext) == list(old) + list(new) and not set(new) & set(old)
    for name, par in old.items():
        assert (ext[name].kind, ext[name].default) == (par.kind, par.default), name
    for name, default in new.items():
        assert ext[name].kind is inspect.Parameter.KEYWORD_ONLY and ext[name].default == default, name
    sm = S.Sampler(None, "euler", 4)
    pixels, mask = torch.zeros(1, 3, 64, 64, dtype=torch.uint8), torch.zeros(1, 64, 64, dtype=torch.uint8)
    noise = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="blend=False"):
        sm.inpaint_ext(None, None, pixels, mask, noise, None, blend=False)
    for bad in (256, -1, 2.0, True):
        with pytest.raises(RuntimeError, match="mask_grow should be"):
            sm.inpaint_ext(None, None, pixels, mask, noise, None, mask_grow=bad)


def _meta(cfg):
    from mixdq_amd.unet import SDXLUNet
    with torch.device("meta"):
        return SDXLUNet(cfg)


def test_inpaint_configs():
    from mixdq_amd.unet import SD15_CONFIG, SD15_INPAINT_CONFIG, SDXL_CONFIG, SDXL_INPAINT_CONFIG
    for cfg, base, total in ((SDXL_INPAINT_CONFIG, SDXL_CONFIG, 2_567_463_684), (SD15_INPAINT_CONFIG, SD15_CONFIG, 859_520_964)):
        assert cfg == dict(base, in_channels=9)
        u = _meta(cfg)
        c0 = cfg["block_out_channels"][0]
        assert u.cond_channels == 5 and tuple(u.conv_in.weight.shape) == (c0, 9, 3, 3)
        assert sum(p.numel() for p in u.conv_in.parameters()) == c0 * 9 * 9 + c0
        assert sum(p.numel() for p in u.parameters()) == total + c0 * 5 * 9
        assert _meta(base).cond_channels == 0
    assert sum(p.numel() for p in _meta(SD15_INPAINT_CONFIG).parameters()) == 859_535_364


@pytest.fixture(scope="module")
def tiny9():
    import bench
    from mixdq_amd.quantize_sdxl import example_inputs
    from mixdq_amd.unet import SDXLUNet, init_synthetic_weights
    unet = init_synthetic_weights(SDXLUNet(dict(bench.TINY_CFG, in_channels=9)), seed=3).double().eval()
    inp = example_inputs(2, 8, "cpu", in_channels=9, seed=4)
    to64 = lambda v: v.double() if torch.is_tensor(v) else {k: t.double() for k, t in v.items()}   # noqa: E731
    return unet, {k: to64(v) for k, v in inp.items()}


def _conv_in_output(unet, *args, **kw):
    seen = []
    h = unet.down_blocks[0].register_forward_pre_hook(lambda mod, a: seen.append(a[0].detach().clone()))
    try:
        with torch.no_grad():
            out = unet(*args, **kw)[0]
    finally:
        h.remove()
    return seen[0], out


def test_split_conv_in_equals_the_concatenated_one_in_float64(tiny9):
    unet, inp = tiny9
    g = torch.Generator().manual_seed(9)
    cat9 = torch.randn(2, 9, 8, 8, generator=g, dtype=torch.float64)
    x4, cond = cat9[:, :4].contiguous(), cat9[:, 4:].contiguous()
    rest = (inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"])
    y_cat, out_cat = _conv_in_output(unet, cat9, *rest)
    term = unet.cond_term(cond)
    assert tuple(term.shape) == (2, 32, 8, 8) and term.dtype == torch.float64
    y_split, out_split = _conv_in_output(unet, x4, *rest, cond_term=term)
    # linearity: the same 81 products per element, summed in another order and rounded to float64
    w = unet.conv_in.weight.detach().numpy()
    _, a = R9.conv3x3_f64(cat9.numpy(), w)
    tol = 1e-12 * a
    err = np.abs(y_cat.numpy() - y_split.numpy())
    assert (err <= tol).all(), f"worst ratio {float((err / tol).max()):.3g}"
    assert float(np.abs(y_cat.numpy()).max()) > 1e-3
    # ... and against the restatement's sums
    sx, sc, b, _ = R9.split_conv_in_f64(x4.numpy(), cond.numpy(), w, unet.conv_in.bias.detach().numpy())
    assert (np.abs(y_split.numpy() - (sx + sc + b)) <= tol).all()
    assert torch.allclose(out_cat, out_split, rtol=1e-9, atol=1e-11)
    # the padded 8-channel form: the padding's content is irrelevant
    cond8 = torch.full((2, 8, 8, 8), 3.5, dtype=torch.float64)
    cond8[:, :5] = cond
    assert torch.equal(unet.cond_term(cond8), term)
    # a weight written in place reaches the next cond_term, in the same storage
    wx, wc = unet._conv_in_split(refresh=False)
    ptrs = (wx.data_ptr(), wc.data_ptr())
    old = unet.conv_in.weight.detach().clone()
    with torch.no_grad():
        unet.conv_in.weight.mul_(-0.5)
    try:
        term2 = unet.cond_term(cond)
        wx2, wc2 = unet._conv_in_split(refresh=False)
        assert (wx2.data_ptr(), wc2.data_ptr()) == ptrs
        assert torch.equal(wx2[:, :4], unet.conv_in.weight[:, :4]) and not wx2[:, 4:].any()
        assert torch.equal(wc2[:, :5], unet.conv_in.weight[:, 4:]) and not wc2[:, 5:].any()
        y2, _ = _conv_in_output(unet, x4, *rest, cond_term=term2)
        y2_cat, _ = _conv_in_output(unet, cat9, *rest)
        assert (np.abs(y2.numpy() - y2_cat.numpy()) <= tol).all() and not torch.equal(y2, y_split)
    finally:
        with torch.no_grad():
            unet.conv_in.weight.copy_(old)
        unet.cond_term(cond)


def test_forward_and_cond_term_refusals(tiny9):
    import bench
    from mixdq_amd.unet import SDXLUNet, init_synthetic_weights
    unet, inp = tiny9
    rest = (inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"])
    x4, cond = torch.zeros(2, 4, 8, 8, dtype=torch.float64), torch.zeros(2, 5, 8, 8, dtype=torch.float64)
    term = unet.cond_term(cond)
    with pytest.raises(RuntimeError, match="needs cond_term"):
        unet(x4, *rest)
    with pytest.raises(RuntimeError, match="cond_term should be"):
        unet(x4, *rest, cond_term=term[:1])                              # wrong rows
    with pytest.raises(RuntimeError, match="cond_term should be"):
        unet(x4, *rest, cond_term=term[:, :16])                          # wrong shape
    with pytest.raises(RuntimeError, match="cond_term should be"):
        unet(x4, *rest, cond_term=term.float())                          # wrong dtype
    with pytest.raises(RuntimeError, match="should have 4 channels"):
        unet(torch.zeros(2, 9, 8, 8, dtype=torch.float64), *rest, cond_term=term)
    with pytest.raises(RuntimeError, match="cond should be"):
        unet.cond_term(cond[:, :4])
    with pytest.raises(RuntimeError, match="cond should be"):
        unet.cond_term(cond.float())
    with pytest.raises(RuntimeError, match="cond should be"):
        unet.cond_term(cond[0])
    plain = init_synthetic_weights(SDXLUNet(bench.TINY_CFG), seed=3).double().eval()
    assert plain.cond_channels == 0
    with pytest.raises(RuntimeError, match="no conditioning channels"):
        plain.cond_term(cond)
    with pytest.raises(RuntimeError, match="no conditioning channels"):
        plain(x4, *rest, cond_term=term)
    with torch.no_grad():
        assert plain(x4, *rest)[0].shape == (2, 4, 8, 8)                 # ... and the 4-channel call is what it was
