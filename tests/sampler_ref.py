"""The sampler step (mixdq_sampler_step; arithmetic: include/mixdq_math.h) restated in numpy float32: every
operation below is one IEEE binary32 round-to-nearest ufunc call, in the specification's order."""
import numpy as np

f32 = np.float32


def step(x, eps_u, eps_c, coef_row, g, noise=None):
    """x fp32, eps_u / eps_c fp16 (eps_c None: rows_per_image == 1), coef_row = (a, b, c, s_next) fp32, noise fp32 or
    None -> (next state fp32, next UNet input fp16)."""
    a, b, c, s_next = (f32(v) for v in coef_row)
    e = eps_u.astype(f32)
    if eps_c is not None:
        e = e + f32(g) * (eps_c.astype(f32) - e)
    y = a * x.astype(f32) + b * e
    if noise is not None:
        y = y + c * noise.astype(f32)
    with np.errstate(over="ignore"):
        return y, (y * s_next).astype(np.float16)


def init(noise, init_scale, input_scale0):
    """The state and the first UNet input of a run."""
    x = noise.astype(f32) * f32(init_scale)
    with np.errstate(over="ignore"):
        return x, (x * f32(input_scale0)).astype(np.float16)
