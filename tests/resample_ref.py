"""The separable resampling kernels (csrc/image.hip; arithmetic: include/mixdq_math.h mixdq_resample_tap,
mixdq_round_u8, mixdq_blend_u8) restated in numpy: every fused multiply-add is tests.exact_inputs.fma32 (one rounding),
in the specification's order -- for every source row the horizontal chain over the taps in order, then the vertical
chain of those FP32 values -- a zero weight is skipped, indices are clamped to the image."""
import numpy as np

from tests.exact_inputs import fma32
from tests.inpaint_ref import mask_set, to_uint8

f32 = np.float32


def tap(acc, w, v):
    """acc where w == 0 (either sign: the operand is never looked at), fl32(w * v + acc) elsewhere."""
    w = np.asarray(w, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(w == 0, np.asarray(acc, f32), fma32(w, v, acc)).astype(f32)


def round_u8(a):
    """NaN -> 0, a <= 0 -> 0, a >= 255 -> 255, otherwise rint (half to even)."""
    a = np.asarray(a, f32)
    with np.errstate(invalid="ignore"):
        r = np.rint(np.minimum(np.maximum(a, f32(0)), f32(255)))
    return np.where(np.isnan(a), f32(0), r).astype(np.uint8)


def blend_u8(m, d, o):
    """(m*d + (255-m)*o + 127) // 255 in integers."""
    m, d, o = (np.asarray(v).astype(np.int64) for v in (m, d, o))
    return ((m * d + (255 - m) * o + 127) // 255).astype(np.uint8)


def source(src, mask=False):
    """Source elements as the FP32 values the chains read."""
    src = np.asarray(src)
    if mask:
        return np.where(mask_set(src), f32(255), f32(0)).astype(f32)
    return src.astype(f32)


def resample(src, xs, wx, ys, wy, mask=False):
    """src [B, C, Hs, Ws] (uint8 / fp16 / fp32), xs int32 [Bt, Wd], wx fp32 [Bt, Wd, Tx], ys int32 [Bt, Hd], wy fp32
    [Bt, Hd, Ty] (Bt 1 or B) -> the FP32 accumulators [B, C, Hd, Wd]."""
    v = source(src, mask)
    B, C, Hs, Ws = v.shape
    Wd, Tx, Hd, Ty = wx.shape[1], wx.shape[2], wy.shape[1], wy.shape[2]
    out = np.empty((B, C, Hd, Wd), dtype=f32)
    for b in range(B):
        tb = 0 if xs.shape[0] == 1 else b
        hor = np.zeros((C, Hs, Wd), dtype=f32)                      # every source row's horizontal value
        for i in range(Tx):
            col = np.clip(xs[tb].astype(np.int64) + i, 0, Ws - 1)
            hor = tap(hor, wx[tb, :, i][None, None, :], v[b][:, :, col])
        acc = np.zeros((C, Hd, Wd), dtype=f32)
        for j in range(Ty):
            row = np.clip(ys[tb].astype(np.int64) + j, 0, Hs - 1)
            acc = tap(acc, wy[tb, :, j][None, :, None], hor[:, row, :])
        out[b] = acc
    return out


def finish(acc, out="u8"):
    """The three destination kinds."""
    return {"u8": round_u8, "u8_unit": to_uint8, "f32": lambda a: np.asarray(a, f32)}[out](acc)


def paste(decoded, original, mask, wins, tables, soft=False):
    """decoded fp16 [B, 3, Hm, Wm], original uint8 [B, 3, H, W], mask [B, H, W], wins [(x0, y0, x1, y1)] per image,
    tables [(xs [w], wx [w, Tx], ys [h], wy [h, Ty])] per image, indexed by the window-relative coordinate -> uint8
    [B, 3, H, W]: blend_u8(m, to_uint8(resized), original) inside each window, the original elsewhere."""
    out = np.array(original, dtype=np.uint8, copy=True)
    for b, (x0, y0, x1, y1) in enumerate(wins):
        xs, wx, ys, wy = (t[None] for t in tables[b])
        assert xs.shape[1] == x1 - x0 and ys.shape[1] == y1 - y0
        acc = resample(decoded[b:b + 1], xs, wx, ys, wy)[0]
        mb = mask[b, y0:y1, x0:x1]
        m = mb.astype(np.int64) if soft else np.where(mask_set(mb), 255, 0)
        out[b, :, y0:y1, x0:x1] = blend_u8(m[None], to_uint8(acc), original[b, :, y0:y1, x0:x1])
    return out
