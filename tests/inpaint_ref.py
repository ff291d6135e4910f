"""Inpainting's arithmetic (include/mixdq_math.h: mixdq_sampler_blend, mixdq_to_uint8) and the two modes of
mixdq_mask_to_latent restated in numpy: every floating-point operation below is one IEEE binary32 round-to-nearest
ufunc call, in the specification's order."""
import numpy as np

f32 = np.float32


def blend(x_new, z, n0, m, p, q):
    """x_new, z, n0, m fp32 (m broadcast by the caller: one value per element), p, q scalars -> fp32:
    k = (p*z) + (q*n0);  ((1 - m) * k) + (m * x_new)."""
    p, q = f32(p), f32(q)
    x_new, z, n0, m = (np.asarray(v, dtype=f32) for v in (x_new, z, n0, m))
    with np.errstate(invalid="ignore", over="ignore"):
        pz = p * z
        qn = q * n0
        k = pz + qn
        keep = f32(1.0) - m
        lhs = keep * k
        rhs = m * x_new
        return lhs + rhs


def kept(z, n0, p, q):
    """What a masked-out (m == 0) element becomes: k = (p*z) + (q*n0)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return f32(p) * np.asarray(z, f32) + f32(q) * np.asarray(n0, f32)


def to_uint8(v):
    """fp16 (or fp32 holding fp16 values) -> uint8: ((v / 2 + 0.5).clamp(0, 1) * 255).round(), half to even; NaN -> 0."""
    v = np.asarray(v).astype(f32)
    with np.errstate(invalid="ignore"):
        t = v * f32(0.5)
        t = t + f32(0.5)
        t = np.minimum(np.maximum(t, f32(0.0)), f32(1.0))
        t = t * f32(255.0)
        t = np.rint(t)
    return np.where(np.isnan(v), f32(0.0), t).astype(np.uint8)


def mask_set(mask):
    """The binarisation: uint8 u >= 128, floats v >= 0.5 (NaN compares false)."""
    mask = np.asarray(mask)
    if mask.dtype == np.uint8:
        return mask >= 128
    with np.errstate(invalid="ignore"):
        return mask.astype(f32) >= f32(0.5)


def mask_to_latent(mask, mode="nearest"):
    """mask [B, H, W] (uint8 / fp16 / fp32) -> fp32 [B, H/8, W/8] of 0.0 / 1.0: pixel (8i, 8j), or any pixel of the
    8x8 block."""
    s = mask_set(mask)
    B, H, W = s.shape
    assert H % 8 == 0 and W % 8 == 0
    if mode == "nearest":
        return s[:, ::8, ::8].astype(f32)
    assert mode == "any"
    return s.reshape(B, H // 8, 8, W // 8, 8).any(axis=(2, 4)).astype(f32)
