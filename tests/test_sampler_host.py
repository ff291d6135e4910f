"""mixdq_amd.sampler's schedules and coefficient tables (host, numpy), and the library's new entry point loaded on
a CPU-only box.

The coefficient check holds the affine form `x' = (a*x + b*e) + c*n` -- tests/sampler_ref.py, float32, driven by the
FP32 coefficient table -- against each scheduler's TEXTBOOK update written out in float64 (predicted x0, derivative,
ancestral split; LCM's boundary-condition scalings), step by step from the same state.  Per element

    |diff| <= 8 * 2^-24 * (|a x| + |b e| + |c n|)  +  2^-24 * (|a x| + |b e| + |c n|)

The first term is the specification's five roundings (two products and a sum, a product and a sum: each at most
2^-24 relative to its result, results bounded by the sum of magnitudes; 8 leaves room for their propagation), the
second the float64 -> FP32 rounding of a, b and c (each 2^-24 relative).  Neither is a measured number.  With
guidance, e is the float64 combination of the FP16 rows: the float32 one is exact or within 2^-24 |e| for FP16 data
and g = 7.5 (11-bit significands, a 4-bit factor), which the first term's slack covers."""
import ctypes

import numpy as np
import pytest

from tests import sampler_ref as R

KINDS = ("euler_ancestral", "euler", "lcm")


def _ac():
    betas = np.linspace(np.sqrt(0.00085), np.sqrt(0.012), 1000, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas)


def test_timestep_spacings():
    from mixdq_amd.sampler import timesteps
    assert timesteps("euler_ancestral", 1).tolist() == [999]
    assert timesteps("euler_ancestral", 4).tolist() == [999, 749, 499, 249]
    assert timesteps("euler", 20).tolist() == list(range(951, 0, -50))
    assert timesteps("euler", 4, spacing="trailing").tolist() == [999, 749, 499, 249]
    assert timesteps("lcm", 4).tolist() == [999, 759, 499, 259]
    with pytest.raises(ValueError):
        timesteps("ddpm", 4)
    with pytest.raises(ValueError):
        timesteps("euler", 4, spacing="linspace")
    with pytest.raises(ValueError):
        timesteps("lcm", 51)


@pytest.mark.parametrize("kind,n", [("euler_ancestral", 1), ("euler_ancestral", 4), ("euler", 20), ("euler", 4)])
def test_sigmas(kind, n):
    from mixdq_amd.sampler import schedule
    s = schedule(kind, n, spacing="trailing" if (kind, n) == ("euler", 4) else None)
    ac = _ac()
    want = np.sqrt((1.0 - ac[s.timesteps]) / ac[s.timesteps])
    assert np.array_equal(s.sigmas[:-1], want) and s.sigmas[-1] == 0.0
    if s.timesteps[0] == 999:
        assert s.sigmas[0] == np.sqrt((1.0 - ac[999]) / ac[999]) and 14.0 < s.sigmas[0] < 15.0
    assert (np.diff(s.sigmas) < 0).all()
    assert s.coef.dtype == np.float32 and s.coef.shape == (n, 4) and s.t_table.dtype == np.float32
    assert s.t_table[:-1].tolist() == [float(t) for t in s.timesteps] and len(s.t_table) == n + 1
    assert s.coef[-1, 3] == 1.0                                   # the final sigma is 0: input scale 1
    want_init = np.sqrt(want[0] ** 2 + 1.0) if kind == "euler_ancestral" else want[0]
    assert s.init_scale == want_init and s.input_scale0 == 1.0 / np.sqrt(want[0] ** 2 + 1.0)
    assert s.uses_noise == (kind == "euler_ancestral" and n > 1)


def test_lcm_schedule_scalars():
    from mixdq_amd.sampler import schedule
    s = schedule("lcm", 4)
    assert s.init_scale == 1.0 and s.input_scale0 == 1.0 and (s.coef[:, 3] == 1.0).all()
    assert s.uses_noise and s.coef[-1, 2] == 0.0 and (s.coef[:-1, 2] > 0).all()
    assert not schedule("lcm", 1).uses_noise


def _textbook_step(kind, s, i, x, e, n):
    """One float64 step of scheduler `kind` at index i of schedule s -- its own formulas, not the affine form."""
    ac = _ac()
    if kind in ("euler", "euler_ancestral"):
        ts = s.timesteps
        s0 = np.sqrt((1.0 - ac[ts[i]]) / ac[ts[i]])
        s1 = np.sqrt((1.0 - ac[ts[i + 1]]) / ac[ts[i + 1]]) if i + 1 < len(ts) else 0.0
        pred_x0 = x - s0 * e
        derivative = (x - pred_x0) / s0
        if kind == "euler":
            return x + derivative * (s1 - s0)
        sigma_up = np.sqrt(s1 ** 2 * (s0 ** 2 - s1 ** 2) / s0 ** 2)
        sigma_down = np.sqrt(s1 ** 2 - sigma_up ** 2)
        return x + derivative * (sigma_down - s0) + n * sigma_up
    t = s.timesteps[i]
    scaled_t = 10.0 * t
    c_skip = 0.5 ** 2 / (scaled_t ** 2 + 0.5 ** 2)
    c_out = scaled_t / np.sqrt(scaled_t ** 2 + 0.5 ** 2)
    x0 = (x - np.sqrt(1.0 - ac[t]) * e) / np.sqrt(ac[t])
    denoised = c_out * x0 + c_skip * x
    if i == s.n_steps - 1:
        return denoised
    t_prev = s.timesteps[i + 1]
    return np.sqrt(ac[t_prev]) * denoised + np.sqrt(1.0 - ac[t_prev]) * n


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("n_steps", [1, 4, 20])
@pytest.mark.parametrize("kind", KINDS)
def test_coefficient_table_against_the_textbook_update(kind, n_steps, guided):
    from mixdq_amd.sampler import schedule
    s = schedule(kind, n_steps)
    rng = np.random.default_rng(1000 * KINDS.index(kind) + 10 * n_steps + guided)
    numel, g = 4099, 7.5
    x, first_in = R.init(rng.standard_normal(numel).astype(np.float32), s.init_scale, s.input_scale0)
    assert first_in.dtype == np.float16 and np.isfinite(first_in).all()
    u = 2.0 ** -24
    for i in range(n_steps):
        eps_u = rng.standard_normal(numel).astype(np.float16)
        eps_c = rng.standard_normal(numel).astype(np.float16) if guided else None
        noise = rng.standard_normal(numel).astype(np.float32) if s.uses_noise else None
        got, nxt = R.step(x, eps_u, eps_c, s.coef[i], g, noise)
        e64 = eps_u.astype(np.float64)
        if guided:
            e64 = e64 + g * (eps_c.astype(np.float64) - e64)
        n64 = noise.astype(np.float64) if noise is not None else np.zeros(numel)
        want = _textbook_step(kind, s, i, x.astype(np.float64), e64, n64)
        a, b, c, s_next = (float(v) for v in s.coef[i])
        mag = np.abs(a * x.astype(np.float64)) + np.abs(b * e64) + np.abs(c * n64)
        diff = np.abs(got.astype(np.float64) - want)
        assert got.dtype == np.float32
        assert (diff <= 8 * u * mag + u * mag).all(), (kind, n_steps, i, float((diff / mag).max() / u))
        # the next input: the FP32 product rounded once more, to FP16
        assert np.array_equal(nxt, (got * np.float32(s_next)).astype(np.float16))
        x = got
    assert np.isfinite(x).all()


def test_library_exports_the_step_and_rejects_bad_arguments():
    """CPU-only load, as tests/test_cabi.py: argument checks run on the host before any launch."""
    from mixdq_amd.build import build
    lib = ctypes.CDLL(build())
    assert hasattr(lib, "mixdq_sampler_step")
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    fn = lib.mixdq_sampler_step
    fn.argtypes = [vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, ctypes.c_float, i64, i32, i64, vp]
    fn.restype = i32
    assert fn(None, None, None, None, 0, None, None, 4, None, None, 0.0, 64, 1, 64, None) == 1
    p = 0x1000                       # (never dereferenced: every call below fails its checks first)
    assert fn(p, p, p, None, 0, p, None, 4, p, p, 0.0, 64, 1, 64, None) == 1          # one null pointer
    assert fn(p, p, p, None, 0, p, p, 4, p, p, 0.0, 64, 3, 64, None) == 1             # rows_per_image not 1 or 2
    assert fn(p, p, p, None, 0, p, p, 4, p, p, 0.0, 64, 0, 64, None) == 1
    assert fn(p, p, p, None, 0, p, p, 4, p, p, 0.0, -1, 1, 64, None) == 1
    assert fn(p, p, p, None, 0, p, p, 0, p, p, 0.0, 64, 1, 64, None) == 1             # no steps
    assert fn(p, p, p, None, 0, p, p, 4, p, p, 0.0, 64, 2, 56, None) == 1             # row blocks overlap
    assert fn(p + 4, p, p, None, 0, p, p, 4, p, p, 0.0, 64, 1, 64, None) == 2         # state not 16-byte aligned
    assert fn(p, p + 2, p, None, 0, p, p, 4, p, p, 0.0, 64, 1, 64, None) == 2
    assert fn(p, p, p, None, 0, p, p, 4, p, p, 0.0, 67, 2, 68, None) == 2             # row_stride % 8
    assert fn(p, p, p, p, 66, p, p, 4, p, p, 0.0, 64, 1, 64, None) == 2               # noise_stride % 4
    lib.mixdq_abi_version.restype = i32
    assert lib.mixdq_abi_version() == 3


def test_sampler_is_exported():
    import mixdq_amd
    from mixdq_amd.sampler import Sampler
    assert mixdq_amd.Sampler is Sampler
    s = Sampler(None, "euler", 3, guidance_scale=5.0)
    assert s.rows_per_image == 2 and Sampler(None, "lcm", 4, guidance_scale=1.0).rows_per_image == 1
