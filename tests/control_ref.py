"""Numpy restatements of the ControlNet glue (include/mixdq_math.h mixdq_control_*, mixdq_hint_unit; mixdq_siluf through
the oracle library) and of the scale-table rule of a run.  Every operation is one numpy float32 operation followed,
where the specification rounds to FP16, by a cast."""
import numpy as np


def _f16(v):
    with np.errstate(all="ignore"):
        return np.asarray(v, np.float32).astype(np.float16)


def control_add(skip, residuals, scales):
    """skip: FP16 array; residuals: K FP16 arrays of its shape; scales: K floats (the table's column of this step).
    Nets in order, a net with scale 0 skipped; every net skipped: skip's own bits."""
    acc = None
    with np.errstate(all="ignore"):
        for r, c in zip(residuals, scales):
            c = np.float32(c)
            if c == 0:
                continue
            t = _f16(r.astype(np.float32) * c)
            acc = t if acc is None else _f16(acc.astype(np.float32) + t.astype(np.float32))
        if acc is None:
            return skip.copy()
        return _f16(skip.astype(np.float32) + acc.astype(np.float32))


def control_add_at(skip, residuals, table, step):
    """... with the scales read from table [K, n_steps] at `step`; a step outside the table: every scale 0."""
    table = np.asarray(table, np.float32)
    col = table[:, step] if 0 <= step < table.shape[1] else np.zeros(table.shape[0], np.float32)
    return control_add(skip, residuals, col)


def silu_f16(x, oracle):
    """f16(mixdq_siluf(f32(x))) by the scalar specification, through the oracle library (one call per distinct value)."""
    L = oracle.lib()
    bits, inv = np.unique(x.view(np.uint16), return_inverse=True)
    with np.errstate(all="ignore"):
        tab = np.array([L.mixdq_oracle_siluf(float(v)) for v in bits.view(np.float16).astype(np.float32)],
                       np.float32).astype(np.float16)
    return tab[inv].reshape(x.shape)


def hint_unit_u8(u):
    """f16(f32(u) / 255.0f): numpy's float32 division is correctly rounded."""
    return _f16(np.asarray(u).astype(np.float32) / np.float32(255.0))


def hint_to_nhwc8(img):
    """img [B, C, H, W] uint8 / float16 / float32 -> FP16 [B, H, W, 8], channels C..7 +0.0."""
    B, C, H, W = img.shape
    out = np.zeros((B, H, W, 8), np.float16)
    v = hint_unit_u8(img) if img.dtype == np.uint8 else _f16(img)
    out[..., :C] = np.transpose(v, (0, 2, 3, 1))
    return out


def scale_table(n_steps, t0, scales, starts, ends):
    """FP32 [K, n_steps]: for a run of m = n_steps - t0 steps that starts at step t0, net k at the run's step j has
    keep = not (j / m < start_k or (j + 1) / m > end_k) (diffusers' controlnet_keep, in Python floats) and
    table[k, t0 + j] = f32(scale_k * keep); every other entry 0."""
    K, m = len(scales), n_steps - t0
    out = np.zeros((K, n_steps), np.float32)
    for k in range(K):
        for j in range(m):
            keep = 1.0 - float(j / m < starts[k] or (j + 1) / m > ends[k])
            out[k, t0 + j] = np.float32(scales[k] * keep)
    return out
