"""The launches the 9-channel inpainting checkpoints add, restated in numpy: mixdq_image_to_nhwc8_f16_masked (the ingest
with the masked pixels blanked), mixdq_inpaint_cond_f16 (mask | latents | zeros in FP16), mixdq_mask_dilate_u8 (the
square maximum of the binarised mask), and the split conv_in in float64."""
import numpy as np

from tests import inpaint_ref as I
from tests import vae_enc_ref as ER

f32 = np.float32


def ingest_masked(image, mask):
    """image [B, C <= 8, H, W] uint8 / fp16 / fp32, mask [B, H, W] uint8 / fp16 / fp32 -> fp16 [B, H, W, 8]: the plain
    ingest (vae_enc_ref.ingest), every channel of a pixel under a set mask value +0.0."""
    out = ER.ingest(image)
    out[I.mask_set(mask)] = np.float16(0.0)
    return out


def inpaint_cond(mask_lat, zl):
    """mask_lat fp32 [B, h, w], zl fp32 [B, h, w, L <= 7] -> fp16 [B, h, w, 8]: f16(mask) | f16(zl) | zeros."""
    B, h, w, L = zl.shape
    assert 1 <= L <= 7 and mask_lat.shape == (B, h, w) and mask_lat.dtype == f32 and zl.dtype == f32
    out = np.zeros((B, h, w, 8), dtype=np.float16)
    with np.errstate(over="ignore"):
        out[..., 0] = mask_lat.astype(np.float16)
        out[..., 1:1 + L] = zl.astype(np.float16)
    return out


def mask_dilate(mask, r):
    """mask [B, H, W] uint8 / fp16 / fp32 -> uint8 [B, H, W]: 255 where any set pixel lies in rows y - r .. y + r and
    columns x - r .. x + r of the same image (clipped at its border), 0 elsewhere.  Written as the definition: one
    pass over the (2r + 1)^2 offsets, each a shifted OR -- not the kernel's two passes."""
    s = I.mask_set(mask)
    B, H, W = s.shape
    out = np.zeros_like(s)
    for dy in range(-min(r, H - 1), min(r, H - 1) + 1):
        ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
        for dx in range(-min(r, W - 1), min(r, W - 1) + 1):
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            out[:, yd, xd] |= s[:, ys, xs]
    return np.where(out, np.uint8(255), np.uint8(0))


def conv3x3_f64(x, w):
    """x [N, C, h, w], w [K, C, 3, 3] (any float dtype) -> (sum, sum of |w||x|) in float64: stride 1, zero padding 1."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    N, C, H, W = x.shape
    xp = np.zeros((N, C, H + 2, W + 2))
    xp[:, :, 1:-1, 1:-1] = x
    s = np.zeros((N, w.shape[0], H, W))
    a = np.zeros_like(s)
    for r in range(3):
        for c in range(3):
            win = xp[:, :, r:r + H, c:c + W]
            s += np.einsum("nchw,kc->nkhw", win, w[:, :, r, c])
            a += np.einsum("nchw,kc->nkhw", np.abs(win), np.abs(w[:, :, r, c]))
    return s, a


def split_conv_in_f64(x, cond, weight, bias):
    """The split conv_in's two exact sums: Sx = conv(x; W[:, :Cx]), Sc = conv(cond; W[:, Cx:]) (+ their |w||x| sums)
    and the bias, all float64, from the operands as given."""
    cx = x.shape[1]
    sx, ax = conv3x3_f64(x, weight[:, :cx])
    sc, ac = conv3x3_f64(cond, weight[:, cx:cx + cond.shape[1]])
    return sx, sc, np.asarray(bias, np.float64)[None, :, None, None], ax + ac
