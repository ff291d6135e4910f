"""InstructPix2Pix's two launches restated in numpy float32 -- mixdq_sampler_guided_eps3 (include/mixdq_math.h), the
three-row guidance of mixdq_sampler_step3, and mixdq_ip2p_cond_f16 (csrc/vae.hip) -- every operation one IEEE binary32
round-to-nearest ufunc call, in the specification's order.  The rest of a step is the existing restatements', which take
the already guided FP32 epsilon in the place of a one-row FP16 one (their `astype(float32)` is then the identity):
tests/sampler_ref.py, multistep_ref.py, inpaint_ref.py; the noise of seeded steps is tests/rng_ref.py's."""
import numpy as np

from tests import inpaint_ref as I
from tests import multistep_ref as M
from tests import sampler_ref as R

f32 = np.float32


def guided_eps3(e_t, e_i, e_u, g, gi):
    """(e_u + g * (e_t - e_i)) + gi * (e_i - e_u): six roundings.  e_t, e_i, e_u: FP16 (or FP32) arrays."""
    et, ei, eu = (np.asarray(e).astype(f32) for e in (e_t, e_i, e_u))
    with np.errstate(invalid="ignore", over="ignore"):
        d_t = et - ei
        p_t = f32(g) * d_t
        s_t = eu + p_t
        d_i = ei - eu
        p_i = f32(gi) * d_i
        return s_t + p_i


def step3(x, e_t, e_i, e_u, row, g, gi, *, noise=None, hist=None, second=False, blend=None):
    """One mixdq_sampler_step3 launch.  row: coef[step] (4 values) or coef8[step] (8 values: then `second` as
    multistep_ref.is_second decides it, and `hist` where it is read); noise: FP32 or None (width 4); blend: None or
    (z, noise0, m, p, q) with m already broadcast to x's shape.  -> (state FP32, next input FP16, new hist or None)."""
    e = guided_eps3(e_t, e_i, e_u, g, gi)
    if len(row) == 8:
        y, p0 = M.step(x, hist, e, None, row, 0.0, second)
        s_next = row[6]
    else:
        y, _ = R.step(x, e, None, row, 0.0, noise)
        p0, s_next = None, row[3]
    if blend is not None:
        z, n0, m, p, q = blend
        y = I.blend(y, z, n0, m, p, q)
    return y, M.scaled_input(y, s_next), p0


def ip2p_cond(moments, rows, scale):
    """moments FP16 [B, h, w, 2L] -> FP16 [rows * B, h, w, 8]: f16(f32(mean) * scale) in channels 0..L-1 of the first
    min(rows, 2) row blocks, +0.0 everywhere else."""
    moments = np.asarray(moments)
    assert moments.dtype == np.float16 and moments.ndim == 4 and moments.shape[3] % 2 == 0 and rows in (1, 3)
    B, h, w, L2 = moments.shape
    L = L2 // 2
    out = np.zeros((rows * B, h, w, 8), dtype=np.float16)
    with np.errstate(over="ignore", invalid="ignore"):
        v = (moments[..., :L].astype(f32) * f32(scale)).astype(np.float16)
    for r in range(min(rows, 2)):
        out[r * B:(r + 1) * B, ..., :L] = v
    return out
