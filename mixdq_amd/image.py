"""The image side of the crop workflow ("inpaint only the masked region"): resize, Gaussian mask blur and the feathered
paste back, all one separable-filter kernel (csrc/image.hip) over tables made here.

The tables are computed in float64 numpy and stored as FP32, exactly as sampler.Schedule makes the sampler's; the
kernel's arithmetic is include/mixdq_math.h (mixdq_resample_tap, mixdq_round_u8, mixdq_blend_u8) and is restated in
numpy bit for bit by tests/resample_ref.py.

    resample_table   PIL's coefficient rule (ImagingResample's precompute_coeffs) for bilinear / bicubic / lanczos3
    gaussian_table   a normalised Gaussian at 1:1, clipped at the image edge
    crop_region      the box around a mask, grown, brought to the model's aspect ratio and kept inside the image
    mask_bbox        one launch + one read-back: the only host synchronisation of the workflow
    resize / blur_mask / paste      the launches

Limits: three filters and the Gaussian; no mask dilation; at most 256 taps per axis (a lanczos3 downscale by 42)."""
import numpy as np

MAX_TAPS = 256


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _bicubic(x, a=-0.5):
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _sinc(x):
    px = np.pi * np.where(x == 0.0, 1.0, x)
    return np.where(x == 0.0, 1.0, np.sin(px) / px)


def _lanczos3(x):
    return np.where((x >= -3.0) & (x < 3.0), _sinc(x) * _sinc(x / 3.0), 0.0)


FILTERS = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0), "lanczos3": (_lanczos3, 3.0)}


def _pack(starts, rows):
    T = max(len(r) for r in rows)
    if T > MAX_TAPS:
        raise RuntimeError(f"image: the filter needs {T} taps, the kernel takes at most {MAX_TAPS}")
    w = np.zeros((len(rows), T), dtype=np.float32)
    for i, r in enumerate(rows):
        w[i, :len(r)] = r
    return np.asarray(starts, dtype=np.int32), w


def resample_table(in_size, lo, hi, out_size, filter="lanczos3"):
    """(start int32 [out_size], weights float32 [out_size, T]): output sample x of an axis is the sum over k of
    weights[x, k] * source[start[x] + k].  The box [lo, hi) of the source (fractional ends allowed) is mapped to
    out_size samples by PIL's rule, in float64: scale = (hi - lo) / out_size, the filter stretched by max(scale, 1),
    window [int(center - support + 0.5), int(center + support + 0.5)) clipped to the IMAGE (not the box: a crop is
    filtered with its real neighbours), weights normalised to sum 1, rows zero-padded to the longest."""
    if filter not in FILTERS:
        raise RuntimeError(f"image: filter should be one of {tuple(FILTERS)}")
    in_size, out_size, lo, hi = int(in_size), int(out_size), float(lo), float(hi)
    if not (in_size >= 1 and out_size >= 1 and 0.0 <= lo < hi <= in_size):
        raise RuntimeError(f"image: box [{lo}, {hi}) should be a non-empty part of [0, {in_size}) and the output "
                           "non-empty")
    fn, base = FILTERS[filter]
    scale = (hi - lo) / out_size
    fs = max(scale, 1.0)
    support = base * fs
    starts, rows = [], []
    for x in range(out_size):
        center = lo + (x + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = fn((np.arange(xmax - xmin, dtype=np.float64) + xmin - center + 0.5) / fs)
        total = w.sum()
        if total != 0.0:
            w = w / total
        starts.append(xmin)
        rows.append(w)
    return _pack(starts, rows)


def gaussian_table(n, sigma):
    """(start int32 [n], weights float32 [n, T]) of a Gaussian blur at 1:1: radius int(3 * sigma + 0.5), w =
    exp(-d^2 / (2 sigma^2)) in float64, the window clipped at the image edge and renormalised -- scipy's
    gaussian_filter1d(mode='constant', truncate=3) divided by the same filter of ones."""
    n, sigma = int(n), float(sigma)
    if not (n >= 1 and sigma > 0.0):
        raise RuntimeError("image: gaussian_table takes n >= 1 and sigma > 0")
    radius = int(3.0 * sigma + 0.5)
    starts, rows = [], []
    for x in range(n):
        xmin, xmax = max(x - radius, 0), min(x + radius + 1, n)
        d = np.arange(xmin, xmax, dtype=np.float64) - x
        w = np.exp(-(d * d) / (2.0 * sigma * sigma))
        starts.append(xmin)
        rows.append(w / w.sum())
    return _pack(starts, rows)


def _ceil_div(a, b):
    return -((-a) // b)


def crop_region(bbox, image_hw, model_hw, pad=32):
    """The window of the image that the crop workflow inpaints, (x0, y0, x1, y1) in integers: `bbox` grown by `pad`
    and clipped to the image; unless it already has the model's aspect ratio (width == ceil(height * Wm / Hm) or height
    == ceil(width * Hm / Wm)), its short side widened to it, centred on the box; shifted back into the image; where the
    image is too small for the widened side, that side is the image's whole extent.  An empty bbox: the whole image."""
    x0, y0, x1, y1 = (int(v) for v in bbox)
    H, W = (int(v) for v in image_hw)
    Hm, Wm = (int(v) for v in model_hw)
    pad = int(pad)
    if not (H >= 1 and W >= 1 and Hm >= 1 and Wm >= 1 and pad >= 0):
        raise RuntimeError("image: crop_region takes positive sizes and pad >= 0")
    if x1 <= x0 or y1 <= y0:
        return (0, 0, W, H)
    x0, y0, x1, y1 = max(x0 - pad, 0), max(y0 - pad, 0), min(x1 + pad, W), min(y1 + pad, H)
    if x1 <= x0 or y1 <= y0:              # (a box outside the image)
        return (0, 0, W, H)
    w, h = x1 - x0, y1 - y0
    if w != _ceil_div(h * Wm, Hm) and h != _ceil_div(w * Hm, Wm):
        if w * Hm < h * Wm:
            nw = _ceil_div(h * Wm, Hm)
            if nw >= W:
                x0, x1 = 0, W
            else:
                x0 = min(max(x0 - (nw - w) // 2, 0), W - nw)
                x1 = x0 + nw
        else:
            nh = _ceil_div(w * Hm, Wm)
            if nh >= H:
                y0, y1 = 0, H
            else:
                y0 = min(max(y0 - (nh - h) // 2, 0), H - nh)
                y1 = y0 + nh
    return (x0, y0, x1, y1)


# ---- device side ----------------------------------------------------------------------------------------------------
_CACHE = {}
_CACHE_MAX = 64


def _cached(key, make):
    """Device tables by (kind, sizes, boxes, filter, device): made and uploaded once."""
    hit = _CACHE.get(key)
    if hit is None:
        if len(_CACHE) >= _CACHE_MAX:
            _CACHE.clear()
        hit = _CACHE[key] = make()
    return hit


def _stack(tables, dev):
    """[(start, weights)] of equal row counts -> (int32 [n_tables, rows], fp32 [n_tables, rows, T]) on the device, the
    narrower tables zero-padded to the widest."""
    import torch
    T = max(w.shape[1] for _, w in tables)
    s = np.stack([st for st, _ in tables])
    w = np.zeros((len(tables), tables[0][1].shape[0], T), dtype=np.float32)
    for i, (_, wi) in enumerate(tables):
        w[i, :, :wi.shape[1]] = wi
    return torch.from_numpy(s).to(dev), torch.from_numpy(w).to(dev)


def _boxes(box, B, H, W, what, integer=False):
    """box: None (the whole image), one (x0, y0, x1, y1) or B of them -> a tuple of 1 or B tuples."""
    if box is None:
        return ((0, 0, W, H),)
    box = tuple(box)
    if len(box) == 4 and not hasattr(box[0], "__len__"):
        box = (box,)
    conv = int if integer else float
    out = tuple(tuple(conv(v) for v in b) for b in box)
    if len(out) not in (1, B) or any(len(b) != 4 for b in out):
        raise RuntimeError(f"{what}: box should be None, one (x0, y0, x1, y1) or one per image")
    for x0, y0, x1, y1 in out:
        if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
            raise RuntimeError(f"{what}: box {(x0, y0, x1, y1)} should be a non-empty part of the {W}x{H} image")
    return out


def mask_bbox(mask):
    """[(x0, y0, x1, y1)] per image of mask [B, H, W] / [B, 1, H, W] (uint8 / FP16 / FP32, any strides): the half-open
    bounding box of the set pixels, (0, 0, 0, 0) where none is.  One launch and one read-back: this WAITS for the GPU."""
    from mixdq_amd import _C
    return [tuple(int(v) for v in row) for row in _C.mask_bbox(mask).cpu().tolist()]


def resize(image, size, box=None, filter="lanczos3", out="u8", mask=False):
    """image [B, C <= 4, H, W] (uint8 / FP16 / FP32, any strides) -> [B, C, size[0], size[1]] in channels-last storage:
    the box (None: the whole image; one (x0, y0, x1, y1), fractional allowed; or B of them) resampled to `size` =
    (height, width) with `filter`, one launch.  out: 'u8' (the accumulator rounded half to even and clamped), 'u8_unit'
    (a [-1, 1] image as pixels, vae.to_uint8's arithmetic) or 'f32'.  mask=True: the source enters as 255 where it is
    set and 0 elsewhere."""
    from mixdq_amd import _C
    B, _, H, W = image.shape
    Hd, Wd = (int(v) for v in size)
    boxes = _boxes(box, B, H, W, "resize")

    def make():
        tx = [resample_table(W, b[0], b[2], Wd, filter) for b in boxes]
        ty = [resample_table(H, b[1], b[3], Hd, filter) for b in boxes]
        return _stack(tx, image.device) + _stack(ty, image.device)
    xs, wx, ys, wy = _cached(("resize", H, W, Hd, Wd, boxes, filter, str(image.device)), make)
    return _C.resample(image, xs, wx, ys, wy, out=out, mask=mask)


def blur_mask(mask, sigma):
    """mask [B, H, W] or [B, 1, H, W] (uint8 / FP16 / FP32, any strides) -> the soft uint8 mask [B, H, W]: 255 where
    the mask is set and 0 elsewhere, blurred by a Gaussian of `sigma` pixels (radius int(3 sigma + 0.5), renormalised
    at the image edge: an all-set mask stays all 255).  One launch."""
    from mixdq_amd import _C
    m = mask if mask.dim() == 4 else mask[:, None]
    H, W = m.shape[-2], m.shape[-1]

    def make():
        return _stack([gaussian_table(W, sigma)], m.device) + _stack([gaussian_table(H, sigma)], m.device)
    xs, wx, ys, wy = _cached(("blur", H, W, float(sigma), str(m.device)), make)
    return _C.resample(m, xs, wx, ys, wy, out="u8", mask=True)[:, 0]


def paste(decoded, original, mask, boxes, filter="lanczos3", soft=False):
    """The crop workflow's last step: decoded FP16 [B, 3, Hm, Wm] is resized to each image's integer window boxes[b] =
    (x0, y0, x1, y1) (one box: every image's) of a CLONE of original (uint8 [B, 3, H, W]) and blended in under `mask`
    ([B, H, W] or [B, 1, H, W] at the original's size; soft=True: uint8 weights, e.g. blur_mask's; otherwise binary by
    mask_to_latent's rule).  Returns uint8 [B, 3, H, W] in channels-last storage; pixels outside the windows, and pixels
    whose weight is 0, are the original's bytes.  One copy and one launch."""
    import torch
    from mixdq_amd import _C
    B, _, Hm, Wm = decoded.shape
    H, W = original.shape[-2], original.shape[-1]
    wins = _boxes(boxes, B, H, W, "paste", integer=True)
    if len(wins) == 1:
        wins = wins * B
    Wt, Ht = max(b[2] - b[0] for b in wins), max(b[3] - b[1] for b in wins)

    def pad_rows(table, n):
        s, w = table
        sp, wp = np.zeros(n, dtype=np.int32), np.zeros((n, w.shape[1]), dtype=np.float32)
        sp[:len(s)], wp[:len(s)] = s, w
        return sp, wp

    def make():
        tx = [pad_rows(resample_table(Wm, 0, Wm, b[2] - b[0], filter), Wt) for b in wins]
        ty = [pad_rows(resample_table(Hm, 0, Hm, b[3] - b[1], filter), Ht) for b in wins]
        win = torch.tensor(wins, dtype=torch.int32).to(decoded.device)
        return _stack(tx, decoded.device) + _stack(ty, decoded.device) + (win,)
    xs, wx, ys, wy, win = _cached(("paste", Hm, Wm, H, W, wins, filter, str(decoded.device)), make)
    if not (torch.is_tensor(original) and original.dtype == torch.uint8 and original.dim() == 4
            and original.shape[0] == B and original.shape[1] == 3 and original.device == decoded.device):
        raise RuntimeError("paste: original should be a uint8 [B, 3, H, W] tensor on decoded's device")
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=decoded.device).permute(0, 3, 1, 2)
    out.copy_(original)
    return _C.resample_paste_u8(decoded, out, mask, win, xs, wx, ys, wy, soft=soft)
