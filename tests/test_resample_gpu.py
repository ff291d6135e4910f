"""The separable resampling kernels on the GPU (csrc/image.hip) against their numpy restatement (tests/resample_ref.py),
bit for bit: mixdq_resample over filters, geometries, channel counts, source dtypes, layouts and destination kinds, its
MASK source, NaN containment and index clamp; mixdq_resample_paste_u8 over windows and mask modes with every FP16
pattern in the decode; mixdq_mask_bbox against torch.nonzero; blur_mask."""
import numpy as np
import pytest
import torch

from tests import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
FILTER_NAMES = ("bilinear", "bicubic", "lanczos3")
NP_DT = {"u8": np.uint8, "f16": np.float16, "f32": np.float32}
# name: (source (H, W), destination (H, W), box (x0, y0, x1, y1) or None)
GEOMETRIES = {"up_fractional_box": ((37, 53), (48, 64), (5.5, 3.25, 41, 30.5)),
              "down4": ((64, 80), (16, 24), None),          # 24 lanczos taps: more source rows than a tile has output rows
              "mixed": ((40, 40), (57, 13), (7.5, 2.25, 33, 39)),
              "identity": ((53, 37), (53, 37), None),
              "tiles": ((130, 70), (261, 139), None)}       # several tiles both ways, with remainders


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(x):
    return x.detach().cpu().contiguous().numpy()


def _same(got, want, what):
    """Bit for bit; two FP32 NaNs count as the same (a NaN's payload is not specified)."""
    g = _np(got) if torch.is_tensor(got) else np.ascontiguousarray(got)
    w = np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {g.shape} {g.dtype} against {w.shape} {w.dtype}"
    if g.dtype == np.float32:
        both = np.isnan(g) & np.isnan(w)
        bad = (g.view(np.uint32) != w.view(np.uint32)) & ~both
    else:
        bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {g.size} elements differ"


def _tables(src_hw, dst_hw, box, name):
    from mixdq_amd.image import resample_table
    (Hs, Ws), (Hd, Wd) = src_hw, dst_hw
    x0, y0, x1, y1 = box if box is not None else (0, 0, Ws, Hs)
    xs, wx = resample_table(Ws, x0, x1, Wd, name)
    ys, wy = resample_table(Hs, y0, y1, Hd, name)
    return xs[None], wx[None], ys[None], wy[None]


def _source(rng, shape, dt):
    if dt == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if dt == "f16":
        return (rng.standard_normal(shape) * 0.7).astype(np.float16)         # a decoded image: beyond [-1, 1] too
    return (rng.random(shape) * 255).astype(f32)


def _layouts(a):
    """A [B, C, H, W] numpy array as GPU tensors of the same values: NCHW, channels-last storage, a strided slice."""
    B, C, H, W = a.shape
    yield "nchw", t(a)
    yield "channels_last", t(a.transpose(0, 2, 3, 1)).permute(0, 3, 1, 2)
    big = torch.zeros((B, C + 1, 2 * H, 3 * W + 1), dtype=t(a).dtype, device=DEV)
    big[:, 1:, ::2, 1::3] = t(a)
    yield "slice", big[:, 1:, ::2, 1::3]


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
@pytest.mark.parametrize("name", FILTER_NAMES)
def test_resize_equals_the_restatement(C, name, geometry):
    from mixdq_amd import image as I
    src_hw, dst_hw, box = GEOMETRIES[geometry]
    tabs = _tables(src_hw, dst_hw, box, name)
    rng = np.random.default_rng(len(name) * 100 + src_hw[0])
    for ch in (1, 3, 4):
        for dt in ("u8", "f16", "f32"):
            src = _source(rng, (2, ch) + src_hw, dt)
            acc = R.resample(src, *tabs)                                        # once: the layouts and kinds share it
            for lname, view in _layouts(src):
                for kind in ("u8", "u8_unit", "f32"):
                    got = I.resize(view, dst_hw, box, name, out=kind)
                    assert tuple(got.shape) == (2, ch) + dst_hw and got.permute(0, 2, 3, 1).is_contiguous()
                    _same(got, R.finish(acc, kind), f"{name} {geometry} C={ch} {dt} {lname} {kind}")


def test_two_boxes_in_one_batch_equal_two_calls():
    """B = 2 with two different boxes: different tap counts, the narrower table zero-padded."""
    from mixdq_amd import image as I
    rng = np.random.default_rng(1)
    src = t(rng.integers(0, 256, (2, 3, 60, 70), dtype=np.uint8))
    boxes = ((2.5, 3, 40, 33.25), (0, 0, 70, 60))                               # an upscale and a downscale to 32x48
    both = I.resize(src, (32, 48), boxes, "lanczos3")
    from mixdq_amd.image import resample_table
    assert resample_table(70, 2.5, 40, 48, "lanczos3")[1].shape[1] != resample_table(70, 0, 70, 48, "lanczos3")[1].shape[1]
    for b in range(2):
        one = I.resize(src[b:b + 1], (32, 48), boxes[b], "lanczos3")
        assert torch.equal(both[b:b + 1], one), b
        tabs = _tables((60, 70), (32, 48), boxes[b], "lanczos3")
        _same(one, R.round_u8(R.resample(_np(src[b:b + 1]), *tabs)), f"box {b}")
    same_box = I.resize(src, (32, 48), (boxes[0],) * 2, "lanczos3")
    assert torch.equal(same_box, I.resize(src, (32, 48), boxes[0], "lanczos3"))


@pytest.mark.parametrize("name", FILTER_NAMES)
def test_identity_returns_the_input_bytes(name):
    from mixdq_amd import image as I
    rng = np.random.default_rng(2)
    src = t(rng.integers(0, 256, (1, 3, 53, 37), dtype=np.uint8))
    assert torch.equal(I.resize(src, (53, 37), None, name), src)


def test_bilinear_2x_upscale_is_the_integer_formula():
    """No FMA emulation needed: the weights are 0.25 / 0.75 (1 at the borders), so 16 * out is an integer below 2^12
    and every partial sum is exact."""
    from mixdq_amd import image as I
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (1, 3, 19, 23), dtype=np.uint8)
    got = _np(I.resize(t(src), (38, 46), None, "bilinear", out="f32"))

    def up(a, axis):                                                            # 4 * the upscaled axis, in integers
        a = np.moveaxis(a, axis, -1)
        n = a.shape[-1]
        prev = np.concatenate([a[..., :1], a[..., :-1]], axis=-1)
        nxt = np.concatenate([a[..., 1:], a[..., -1:]], axis=-1)
        out = np.empty(a.shape[:-1] + (2 * n,), dtype=np.int64)
        out[..., 0::2] = 3 * a + prev
        out[..., 1::2] = 3 * a + nxt
        return np.moveaxis(out, -1, axis)
    want = up(up(src.astype(np.int64), 3), 2)
    assert np.array_equal(got * f32(16), want.astype(f32)) and np.array_equal(got * 16 % 1, np.zeros_like(got))


@pytest.mark.parametrize("dt", ["u8", "f16", "f32"])
def test_mask_source(dt):
    """MASK: an element enters as 255 where it is set (u >= 128, v >= 0.5; NaN is not) and 0 elsewhere."""
    from mixdq_amd import image as I
    rng = np.random.default_rng(4)
    if dt == "u8":
        vals = np.array([0, 1, 127, 128, 255, 200], dtype=np.uint8)
    else:
        h = np.float16(0.5)
        vals = np.array([0.0, 0.25, np.nextafter(h, np.float16(0)), h, np.nextafter(h, np.float16(1)), 1.0, np.nan, -1.0,
                         np.inf, -np.inf], dtype=NP_DT[dt])
    m = rng.choice(vals, size=(2, 1, 37, 53))
    tabs = _tables((37, 53), (48, 64), (5.5, 3.25, 41, 30.5), "bilinear")
    want = R.round_u8(R.resample(m, *tabs, mask=True))
    assert 0 < (want == 0).sum() and 0 < (want == 255).sum() and ((want > 0) & (want < 255)).any()
    for lname, view in _layouts(m):
        _same(I.resize(view, (48, 64), (5.5, 3.25, 41, 30.5), "bilinear", mask=True), want, f"{dt} {lname}")
    hard = np.where(R.mask_set(m), 255, 0).astype(np.uint8)                     # == VALUE mode on the binarised mask
    _same(I.resize(t(hard), (48, 64), (5.5, 3.25, 41, 30.5), "bilinear"), want, "binarised first")
    ident = I.resize(t(m), (37, 53), None, "bilinear", mask=True)
    assert torch.equal(ident, t(hard))


def test_nan_beside_the_box_stays_out(C):
    """An FP32 source with NaN / inf beside a box: pixels whose real taps do not cover them stay clean -- the
    zero-padded taps of the shorter table rows and weights that are zero never multiply them."""
    from mixdq_amd import image as I
    from mixdq_amd.image import resample_table
    rng = np.random.default_rng(5)
    src = (rng.random((1, 1, 40, 40)) * 255).astype(f32)
    box, out = (8.3, 8.3, 31.7, 31.7), (9, 9)                                   # a 2.6x downscale: 5 or 6 taps a row
    xs, wx = resample_table(40, 8.3, 31.7, 9, "bilinear")
    used = np.array([np.flatnonzero(r)[-1] + 1 for r in wx])
    used_lo, used_hi = int(xs.min()), int((xs + used).max())
    assert used.min() < wx.shape[1] and 0 < used_lo and used_hi < 40            # padded taps; room beside the taps
    clean = R.resample(src, xs[None], wx[None], xs[None], wx[None])
    src[:, :, :used_lo, :] = np.nan
    src[:, :, used_hi:, :] = np.inf
    src[:, :, :, :used_lo] = -np.inf
    src[:, :, :, used_hi:] = np.nan
    got = I.resize(t(src), out, box, "bilinear", out="f32")
    assert bool(torch.isfinite(got).all())
    _same(got, clean, "NaN outside the real taps")
    src[0, 0, 20, 20] = np.nan                                                  # inside the taps it does reach pixels
    bad = torch.isnan(I.resize(t(src), out, box, "bilinear", out="f32"))
    assert 0 < int(bad.sum()) < 81
    # hand-made: every zero tap (padding, +0 and -0 weights) points AT a NaN or inf, every other tap beside them
    nan, inf = np.nan, np.inf
    line = np.array([1, 2, 3, 4, nan, inf, -inf, nan, 5, 6, 7, 8], dtype=f32)
    with np.errstate(invalid="ignore"):
        img = (line[:, None] * f32(0.5) + line[None, :])[None, None].astype(f32) # NaN / inf in rows and columns 4..7
    img[0, 0, :4, :4] = np.arange(16, dtype=f32).reshape(4, 4)
    start = np.array([[2, 6, 3, 8]], dtype=np.int32)
    w = np.array([[[0.5, 0.5, 0.0], [0.0, -0.0, 1.0], [1.0, -0.0, 0.0], [0.25, 0.5, 0.25]]], dtype=f32)
    got = C.resample(t(img), t(start), t(w), t(start), t(w), out="f32")
    want = R.resample(img, start, w, start, w)
    assert np.isfinite(want).all() and float(want[0, 0, 0, 0]) == (10 + 11 + 14 + 15) / 4
    _same(got, want, "zero taps on NaN")


def test_out_of_range_and_scattered_tables_are_clamped(C):
    """A deliberately bad start table: indices are clamped to the image (wrong pixels, no fault, OK), also where the
    rows of a tile lie further apart than their windows together (each output row then walks its own window)."""
    rng = np.random.default_rng(6)
    Hs, Ws, Hd, Wd, T = 21, 33, 19, 70, 5
    src = rng.integers(0, 256, (2, 3, Hs, Ws), dtype=np.uint8)
    imin, imax = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    xs = rng.integers(-4, Ws + 2, (1, Wd)).astype(np.int32)
    xs[0, :6] = [imin, imax, -1000, 10 ** 9, -T, Ws - 1]
    ys = rng.integers(-3, Hs + 1, (1, Hd)).astype(np.int32)                     # unsorted: rows of a tile far apart
    ys[0, :4] = [imax, imin, Hs - 2, -2]
    ys[0, 8:16] = [0, Hs - 1, 0, Hs - 1, 1, Hs - 3, 2, Hs - 2]                  # one tile whose span exceeds 8 windows
    wx = rng.standard_normal((1, Wd, T)).astype(f32)
    wy = rng.standard_normal((1, Hd, 2)).astype(f32)
    wx[0, ::7, 2] = 0.0
    want = R.resample(src, xs, wx, ys, wy)
    got = C.resample(t(src), t(xs), t(wx), t(ys), t(wy), out="f32")
    _same(got, want, "clamped")
    ys_sorted = np.sort(np.clip(ys, 0, Hs - 1), axis=1)                         # ... and a streaming one
    _same(C.resample(t(src), t(xs), t(wx), t(ys_sorted), t(wy), out="f32"), R.resample(src, xs, wx, ys_sorted, wy), "sorted")
    with pytest.raises(RuntimeError, match="tables should"):
        C.resample(t(src), t(xs), t(wx[:, :-1]), t(ys), t(wy))
    with pytest.raises(RuntimeError, match="tables should"):
        C.resample(t(src), t(xs).long(), t(wx), t(ys), t(wy))
    with pytest.raises(RuntimeError, match="1 to 4 channels"):
        C.resample(t(np.zeros((1, 5, 4, 4), np.uint8)), t(xs), t(wx), t(ys), t(wy))


# ---- the paste ---------------------------------------------------------------------------------------------------
H0, W0, HM, WM = 83, 101, 112, 112
WINS = ((10, 7, 70, 60), (0, 0, 101, 83))


@pytest.fixture(scope="module")
def paste_case():
    """The decode holds every FP16 bit pattern once (in order: the NaNs and the huge values lie together and spoil a
    few rows, the rest of the image is ordinary), then values around [-1, 1]; the reference accumulators' tables."""
    from mixdq_amd.image import resample_table
    rng = np.random.default_rng(7)
    n = 2 * 3 * HM * WM
    flat = np.empty(n, dtype=np.float16)
    flat[:65536] = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    flat[65536:] = (rng.standard_normal(n - 65536) * 0.7).astype(np.float16)
    decoded = np.roll(flat, 5000).reshape(2, 3, HM, WM)
    original = rng.integers(0, 256, (2, 3, H0, W0), dtype=np.uint8)
    tables = []
    for x0, y0, x1, y1 in WINS:
        tables.append(resample_table(WM, 0, WM, x1 - x0, "lanczos3") + resample_table(HM, 0, HM, y1 - y0, "lanczos3"))
    return decoded, original, tables


def _outside(wins, shape):
    out = np.ones(shape, dtype=bool)
    for b, (x0, y0, x1, y1) in enumerate(wins):
        out[b, :, y0:y1, x0:x1] = False
    return out


def test_paste_soft_mask(paste_case):
    from mixdq_amd import image as I
    decoded, original, tables = paste_case
    rng = np.random.default_rng(8)
    mask = rng.integers(0, 256, (2, H0, W0), dtype=np.uint8)
    mask[:, 20:30, :] = 0                                                       # planted runs of both ends
    mask[:, 40:50, 5:90] = 255
    mask[:, :, 33:37] = 0
    want = R.paste(decoded, original, mask, WINS, tables, soft=True)
    orig_d = t(original)
    keep = orig_d.clone()
    for oname, orig_view in (("nchw", orig_d), ("channels_last", t(original.transpose(0, 2, 3, 1)).permute(0, 3, 1, 2))):
        for mname, m in (("bhw", t(mask)), ("b1hw", t(mask)[:, None]),
                         ("transposed", t(mask.transpose(0, 2, 1)).transpose(1, 2))):
            got = I.paste(t(decoded), orig_view, m, WINS, "lanczos3", soft=True)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 3, H0, W0)
            assert got.permute(0, 2, 3, 1).is_contiguous()
            _same(got, want, f"soft {oname} {mname}")
    assert torch.equal(orig_d, keep)                                            # the caller's original is not touched
    g = _np(got)
    out = _outside(WINS, g.shape)
    assert out.any() and np.array_equal(g[out], original[out])                  # nothing outside a window is written
    m3 = np.broadcast_to(mask[:, None], g.shape)
    assert np.array_equal(g[m3 == 0], original[m3 == 0])                        # weight 0: the original's byte
    acc = R.resample(decoded[1:], *(tb[None] for tb in tables[1]))              # image 1's window is the whole image
    full = (m3[1] == 255)
    assert full.sum() > 1000 and np.array_equal(g[1][full], R.to_uint8(acc[0])[full])
    assert (g != original).any() and np.isnan(acc).any() and not np.isnan(acc).all()
    one = I.paste(t(decoded), orig_d, t(mask), WINS[0], "lanczos3", soft=True)  # one box: every image's
    _same(one[:1], want[:1], "one box for the batch")
    with pytest.raises(RuntimeError, match="soft mask should be uint8"):
        I.paste(t(decoded), orig_d, t(mask).float(), WINS, "lanczos3", soft=True)
    with pytest.raises(RuntimeError, match="box"):
        I.paste(t(decoded), orig_d, t(mask), (0, 0, W0 + 1, H0), "lanczos3")


@pytest.mark.parametrize("dt", ["u8", "f16", "f32"])
def test_paste_binary_mask(paste_case, dt):
    from mixdq_amd import image as I
    decoded, original, tables = paste_case
    rng = np.random.default_rng(9)
    if dt == "u8":
        vals = np.array([0, 127, 128, 255], dtype=np.uint8)
    else:
        h = np.float16(0.5)
        vals = np.array([0.0, np.nextafter(h, np.float16(0)), h, 1.0, np.nan, -1.0], dtype=NP_DT[dt])
    mask = rng.choice(vals, size=(2, H0, W0))
    want = R.paste(decoded, original, mask, WINS, tables)
    got = I.paste(t(decoded), t(original), t(mask), WINS, "lanczos3")
    _same(got, want, f"binary {dt}")
    g, set_px = _np(got), np.broadcast_to(R.mask_set(mask)[:, None], want.shape)
    assert np.array_equal(g[~set_px], original[~set_px])
    inside = ~_outside(WINS, g.shape)
    acc = R.resample(decoded[1:], *(tb[None] for tb in tables[1]))               # image 1's window: the whole image
    assert np.array_equal(g[1][set_px[1]], R.to_uint8(acc[0])[set_px[1]])       # m = 255: the resampled decode's pixel
    assert (set_px & inside).any() and (set_px & ~inside).any()                 # a set pixel outside its window stays


# ---- the bounding box ---------------------------------------------------------------------------------------------
def _bbox_ref(mask_bool):
    out = []
    for m in mask_bool:
        nz = torch.nonzero(m)
        if nz.numel() == 0:
            out.append((0, 0, 0, 0))
        else:
            out.append((int(nz[:, 1].min()), int(nz[:, 0].min()), int(nz[:, 1].max()) + 1, int(nz[:, 0].max()) + 1))
    return out


@pytest.mark.parametrize("dt", ["u8", "f16", "f32"])
def test_mask_bbox(C, dt):
    from mixdq_amd import image as I
    rng = np.random.default_rng(10)
    H, W = 67, 1300                                                             # wider than the workgroup has lanes
    m = np.zeros((8, H, W), dtype=NP_DT[dt])
    lo, hi = (127, 128) if dt == "u8" else (np.nextafter(np.float16(0.5), np.float16(0)), 0.5)
    m[:] = lo                                                                    # just under the threshold: not set
    if dt != "u8":
        m[:, ::5, ::7] = np.nan
    for b, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        m[b, y, x] = hi                                                          # a single pixel in each corner
    m[5][rng.random((H, W)) < 0.001] = hi                                        # a random one; 4 and 6 stay empty
    m[7, 11:40, 1030:1100] = hi
    want = _bbox_ref(torch.from_numpy(R.mask_set(m)))
    assert want[0] == (0, 0, 1, 1) and want[3] == (W - 1, H - 1, W, H) and want[4] == (0, 0, 0, 0)
    assert want[7] == (1030, 11, 1100, 40)
    assert I.mask_bbox(t(m)) == want
    assert I.mask_bbox(t(m)[:, None]) == want
    dev = C.mask_bbox(t(m))
    assert dev.dtype == torch.int32 and tuple(dev.shape) == (8, 4) and dev.is_cuda
    big = torch.zeros((8, 2 * H, 3 * W + 1), dtype=t(m).dtype, device=DEV)
    big[:, ::2, 1::3] = t(m)
    assert I.mask_bbox(big[:, ::2, 1::3]) == want                                # a strided slice
    tr = t(m.transpose(0, 2, 1))                                                 # [B, W, H]: the other axis long
    assert I.mask_bbox(tr) == [(y0, x0, y1, x1) for x0, y0, x1, y1 in want]
    assert I.mask_bbox(t(m[:0])) == []


# ---- the blur -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 1.0, 4.0])
def test_blur_mask(sigma):
    from mixdq_amd import image as I
    from mixdq_amd.image import gaussian_table
    rng = np.random.default_rng(11)
    m = np.zeros((2, 37, 53), dtype=np.uint8)
    m[0, 10:25, 20:40] = 255
    m[0, 0:3, 0:4] = 200                                                        # at the corner: the clipped windows
    m[1] = rng.choice(np.array([0, 127, 128, 255], dtype=np.uint8), size=(37, 53))
    xs, wx = gaussian_table(53, sigma)
    ys, wy = gaussian_table(37, sigma)
    want = R.round_u8(R.resample(m[:, None], xs[None], wx[None], ys[None], wy[None], mask=True))[:, 0]
    got = I.blur_mask(t(m), sigma)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 37, 53)
    _same(got, want, f"sigma {sigma}")
    _same(I.blur_mask(t(m)[:, None], sigma), want, "[B, 1, H, W]")
    _same(I.blur_mask(t(m).float() / 255, sigma), want, "an FP32 mask")
    w = want[0].astype(int)
    assert w[36, 0] == 0 and ((w > 0) & (w < 255)).any() and (sigma > 1 or w[17, 30] == 255)     # a feathered edge
    full = torch.full((1, 37, 53), 255, dtype=torch.uint8, device=DEV)
    assert bool((I.blur_mask(full, sigma) == 255).all())                         # renormalised at the image edge
