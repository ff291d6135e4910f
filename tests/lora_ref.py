"""numpy restatement (float64) of mixdq_lora_requant's arithmetic, include/mixdq_math.h mixdq_lora_*: the only reference of
the LoRA tests.  Arrays are in LOGICAL row order; `stored()` applies a row map."""
import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64


def merged(W, B, A, svec):
    """(W' in float64, |W| + sum_r |Bs A|: the magnitude the FP32 accumulation bound is stated in).  Bs = f16(svec *
    f32(Bcat)): the exact product (float64 holds it) rounded ONCE; exactly 0 where svec == 0."""
    bs = (svec.astype(F64)[None, :] * B.astype(F64)).astype(F16).astype(F64)
    bs[:, svec == 0] = 0
    return W.astype(F64) + bs @ A.astype(F64), np.abs(W.astype(F64)) + np.abs(bs) @ np.abs(A.astype(F64))


def pack_w4(q):
    """MIXDQ_FLAG_W4: within 8 consecutive k, byte j holds k[j] in the high and k[4 + j] in the low nibble."""
    g = q.reshape(q.shape[0], -1, 2, 4).astype(np.int16)
    return (((g[:, :, 0] & 15) << 4) | (g[:, :, 1] & 15)).astype(np.uint8).reshape(q.shape[0], -1).view(np.int8)


def requant(W, B, A, svec, mode, rule, bits, old_scales, act_scale, act_zp, tap_len, delta=None):
    """Everything the launch writes for one layer, plus the float64 quotient and merged()'s magnitude.  mode 'int8' | 'w4' |
    'f16'; rule 'keep' | 'absmax'; `delta`: these per-row scales instead of the rule's (the GPU's own, in the random test)."""
    wp, mag = merged(W, B, A, svec)
    if mode == "f16":
        return dict(out=wp.astype(F16), wp=wp, mag=mag)
    qmax = 2 ** (bits - 1) - 1
    if delta is None:
        delta = old_scales.astype(F32)
        if rule == "absmax":
            mx = np.abs(wp).max(axis=1).astype(F32)
            delta = np.where(mx > 0, mx / F32(qmax), delta).astype(F32)
    # an 8-bit quantizer multiplies by the FP32 reciprocal (torch.quantize_per_channel), a narrower one divides (Path A)
    quot = wp * (F32(1) / delta).astype(F64)[:, None] if bits == 8 else wp / delta.astype(F64)[:, None]
    q = np.clip(np.rint(quot.astype(F32)), -qmax - 1, qmax).astype(np.int8)
    taps = q.reshape(q.shape[0], -1, tap_len).astype(np.int64).sum(axis=2)
    return dict(out=q if mode == "int8" else pack_w4(q), q=q, quot=quot, wp=wp, mag=mag, weight_scales=delta,
                wsum=taps.astype(F32), bias0=taps.sum(axis=1).astype(F32) * F32(act_zp),
                scale=delta * F32(act_scale))


def stored(a, row_map):
    """Rows of `a` (logical order) where the launch writes them: out[row_map[n]] = a[n]."""
    out = np.empty_like(a)
    out[row_map] = a
    return out
