"""The multistep sampler on the host (no GPU): `multistep_table` against DPM-Solver++ 2M written from its own log / exp
formulas (tests/multistep_ref.py) in float64, the table's structure, the Karras ladder, the solver's ORDER OF
CONVERGENCE on a model whose exact answer is known, the 'ddim' table against its formula and against the first-order
2M map (DPM-Solver++ 1 is DDIM), the two new functions of include/mixdq_math.h -- compiled by the host compiler
without contraction into a stand-alone program -- against their numpy restatement bit for bit, and the argument checks
of the two new entry points through the C ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import multistep_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, ALIGNMENT = 0, 1, 2


def _ac():
    betas = np.linspace(np.sqrt(0.00085), np.sqrt(0.012), 1000, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas)


def _schedule(variant, n):
    from mixdq_amd.sampler import Schedule
    if variant == "karras":
        return Schedule("dpmpp_2m", n, karras=True)
    return Schedule("dpmpp_2m", n, spacing=variant)


# ---- the table is the solver ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [0, 4])
@pytest.mark.parametrize("variant", ["leading", "trailing", "karras"])
def test_table_equals_the_direct_solver(variant, start):
    """Both in float64 on the Gaussian model from the same state: within 1e-12 of max|x| (the two differ only in how
    the same real numbers are grouped; a float64 rounding is 1.1e-16 and a run has 10 steps of a handful each)."""
    from mixdq_amd.sampler import multistep_table
    s = _schedule(variant, 10)
    tab = multistep_table(s.sigmas)
    rng = np.random.default_rng(10 * start + len(variant))
    x = rng.standard_normal(257) * 1.5
    for scale in (0.5, 2.0):
        model = M.gaussian_model(scale)
        want = M.direct_2m(model, x, s.sigmas, start)
        got = M.table_2m(model, x, tab, s.sigmas, start)
        diff = float(np.abs(got - want).max())
        print(f"{variant} start {start} s {scale}: max diff {diff:.3e}, max|x| {np.abs(want).max():.3e}")
        assert diff <= 1e-12 * float(np.abs(x).max())
        assert not np.array_equal(want, M.direct_2m(model, x, s.sigmas, start, second_order=False))


@pytest.mark.parametrize("variant", ["leading", "trailing", "karras"])
@pytest.mark.parametrize("n", [1, 2, 3, 10])
def test_table_structure(variant, n):
    from mixdq_amd.sampler import multistep_table
    s = _schedule(variant, n)
    tab = multistep_table(s.sigmas)
    assert tab.dtype == np.float64 and tab.shape == (n, 8)
    assert s.order == 2 and not s.uses_noise and s.init_scale == 1.0 and s.input_scale0 == 1.0
    assert s.coef.dtype == np.float32 and np.array_equal(s.coef, tab.astype(np.float32))
    assert len(s.sigmas) == n + 1 and s.sigmas[-1] == 0.0 and (np.diff(s.sigmas) < 0).all()
    assert (tab[:, 6] == 1.0).all() and (tab[:, 7] == 0.0).all()                  # s_next, the pad
    for i in (0, n - 1):
        assert tab[i, 5] == 0.0 and tab[i, 4] == tab[i, 3]
    assert tab[-1, 2] == 0.0 and tab[-1, 3] == 1.0
    if n <= 2:
        assert (tab[:, 5] == 0.0).all()                                           # all first-order
    else:
        assert (tab[1:-1, 5] < 0.0).all() and (tab[1:-1, 4] > tab[1:-1, 3]).all()
    alphas = 1.0 / np.sqrt(s.sigmas[:-1] ** 2 + 1.0)
    assert np.array_equal(tab[:, 0], 1.0 / alphas) and np.array_equal(tab[:, 1], -s.sigmas[:-1])    # u = 1 / alpha
    assert s.t_table.dtype == np.float32 and s.t_table[:-1].tolist() == [float(t) for t in s.timesteps]
    # the start scalars: VP add_noise at that sigma, input scale 1; blend is built from them
    for t0 in range(n):
        sig = s.sigmas[t0]
        alpha = 1.0 / np.sqrt(sig ** 2 + 1.0)
        assert s.start(t0) == (float(alpha), float(sig * alpha), 1.0)                 # sigma_hat = sigma * alpha
    assert s.blend.shape == (n, 2) and s.blend[-1].tolist() == [1.0, 0.0]
    for i in range(n - 1):
        assert s.blend[i].tolist() == [float(np.float32(v)) for v in s.start(i + 1)[:2]]


def test_orders_and_refusals():
    from mixdq_amd.sampler import Sampler, Schedule, multistep_table, timesteps
    for kind in ("euler_ancestral", "euler", "lcm", "ddim"):
        assert Schedule(kind, 4).order == 1 and Schedule(kind, 4).coef.shape == (4, 4)
    assert Schedule("dpmpp_2m", 4).order == 2 and Schedule("dpmpp_2m", 4).coef.shape == (4, 8)
    sm = Sampler(None, "dpmpp_2m", 6, guidance_scale=7.5, karras=True)
    assert sm.schedule.order == 2 and sm.rows_per_image == 2
    assert np.array_equal(sm.schedule.coef, Schedule("dpmpp_2m", 6, karras=True).coef)
    for kind in ("euler", "euler_ancestral", "lcm", "ddim"):
        with pytest.raises(ValueError, match="karras"):
            Schedule(kind, 4, karras=True)
    with pytest.raises(ValueError, match="karras"):
        Schedule("dpmpp_2m", 4, spacing="trailing", karras=True)
    for kind in ("ddim", "dpmpp_2m"):
        with pytest.raises(ValueError):
            timesteps(kind, 4, spacing="linspace")
    with pytest.raises(ValueError):
        timesteps("ddpm", 4)
    for bad in ([1.0, 2.0, 0.0], [2.0, 1.0], [2.0, 1.0, 1.0, 0.0], [0.0], [1.0, -1.0, 0.0]):
        with pytest.raises(ValueError, match="sigmas"):
            multistep_table(bad)


# ---- Karras sigmas -------------------------------------------------------------------------------------------------
def test_karras_ladder():
    from mixdq_amd.sampler import Schedule, timesteps
    s = Schedule("dpmpp_2m", 5, karras=True)
    assert np.isclose(s.sigmas[0], 14.6146, rtol=1e-5) and np.isclose(s.sigmas[4], 0.029167, rtol=1e-5)
    ac = _ac()
    rho = 7.0
    hi, lo = np.sqrt((1 - ac[999]) / ac[999]), np.sqrt((1 - ac[0]) / ac[0])
    want = (hi ** (1 / rho) + np.linspace(0, 1, 5) * (lo ** (1 / rho) - hi ** (1 / rho))) ** rho
    assert np.allclose(s.sigmas[:-1], want, rtol=1e-12, atol=0) and s.sigmas[-1] == 0.0
    assert s.timesteps.tolist() == [999, 786, 427, 59, 0]
    assert timesteps("dpmpp_2m", 5, karras=True).tolist() == [999, 786, 427, 59, 0]
    assert timesteps("dpmpp_2m", 20).tolist() == timesteps("euler", 20).tolist()
    assert timesteps("dpmpp_2m", 4, spacing="trailing").tolist() == [999, 749, 499, 249]
    lead = Schedule("dpmpp_2m", 20)
    assert np.array_equal(lead.sigmas[:-1], np.sqrt((1 - ac[lead.timesteps]) / ac[lead.timesteps]))


# ---- order of convergence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0.5, 1.0, 2.0])
def test_second_order_convergence_on_the_gaussian_model(s):
    """Data ~ N(0, s^2): the exact end point of the probability-flow ODE from x_T is known in closed form.  On the
    ladder geomspace(10, 1e-3, n) + [0] halving the step divides the error of a second-order method by 4 and of a
    first-order one by 2: the table's ratios must be >= 3.5, and <= 2.2 with its second-order terms removed."""
    from mixdq_amd.sampler import multistep_table
    x_T = np.linspace(-3.0, 3.0, 13)
    model = M.gaussian_model(s)
    err = {True: [], False: []}
    for n in (32, 64, 128):
        sig = np.concatenate([np.geomspace(10.0, 1e-3, n), [0.0]])
        tab = multistep_table(sig)
        exact = M.gaussian_exact(x_T, sig[0], s)
        for second in (True, False):
            err[second].append(float(np.abs(M.table_2m(model, x_T, tab, sig, second_order=second) - exact).max()))
    r2 = [err[True][i] / err[True][i + 1] for i in range(2)]
    r1 = [err[False][i] / err[False][i + 1] for i in range(2)]
    print(f"s {s}: second-order errors {err[True]} ratios {r2}; first-order errors {err[False]} ratios {r1}")
    assert min(r2) >= 3.5, r2
    assert max(r1) <= 2.2, r1
    assert err[True][0] < err[False][0]


# ---- ddim ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", ["leading", "trailing"])
@pytest.mark.parametrize("n", [1, 4, 20])
def test_ddim_table(n, spacing):
    from mixdq_amd.sampler import Schedule, multistep_table, timesteps
    s = Schedule("ddim", n, spacing=spacing)
    ac = _ac()
    ts = s.timesteps
    assert ts.tolist() == timesteps("euler", n, spacing=spacing).tolist() == timesteps("ddim", n, spacing).tolist()
    assert s.order == 1 and not s.uses_noise and s.init_scale == 1.0 and s.input_scale0 == 1.0 and s.sigmas is None
    want = np.zeros((n, 4))
    for i, t in enumerate(ts):
        prev = t - 1000 // n if spacing == "leading" else (ts[i + 1] if i + 1 < n else -1)
        ac_prev = ac[prev] if prev >= 0 else ac[0]
        sa, s1a, sp = np.sqrt(ac[t]), np.sqrt(1 - ac[t]), np.sqrt(ac_prev)
        want[i] = (sp / sa, np.sqrt(1 - ac_prev) - sp * s1a / sa, 0.0, 1.0)
    assert s.coef.dtype == np.float32 and np.array_equal(s.coef, want.astype(np.float32))
    last_prev = ts[-1] - 1000 // n if spacing == "leading" else -1
    assert last_prev < 0                                          # ... so the last row steps to ac[0], not to 1
    assert s.coef[-1, 0] == np.float32(np.sqrt(ac[0]) / np.sqrt(ac[ts[-1]]))
    for t0 in range(n):                                           # start(t0) is lcm's: DDPM's add_noise
        assert s.start(t0) == (float(np.sqrt(ac[ts[t0]])), float(np.sqrt(1 - ac[ts[t0]])), 1.0)
    # DPM-Solver++ 1 is DDIM: over the sigmas of a timestep pair the first-order 2M map x' = A x + B1 (u x + v e) is
    # the ddim row, in float64
    if n > 1:
        pairs = [(t, t - 1000 // n if spacing == "leading" else ts[i + 1]) for i, t in enumerate(ts[:-1])]
        for i, (t, prev) in enumerate(pairs):
            sig = np.sqrt((1 - ac[[t, prev]]) / ac[[t, prev]])
            u, v, A, B1 = multistep_table(np.concatenate([sig, [0.0]]))[0, :4]
            assert abs(A + B1 * u - want[i, 0]) <= 1e-12 and abs(B1 * v - want[i, 1]) <= 1e-12, (i, t, prev)


# ---- the arithmetic specification ----------------------------------------------------------------------------------
_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "mixdq_math.h"

/* spec IN OUT x0|2m: IN holds FP32 tuples -- x0: (x, e, u, v); 2m: (x, x0, h, A, B, D) -- OUT one FP32 per tuple */
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 3;
  float t[6];
  if (argv[3][0] == 'x') {
    while (fread(t, 4, 4, in) == 4) {
      const float r = mixdq_sampler_x0(t[0], t[1], t[2], t[3]);
      fwrite(&r, 4, 1, out);
    }
  } else {
    while (fread(t, 4, 6, in) == 6) {
      const float r = mixdq_sampler_update_2m(t[0], t[1], t[2], t[3], t[4], t[5]);
      fwrite(&r, 4, 1, out);
    }
  }
  fclose(in);
  return fclose(out) ? 4 : 0;
}
"""


@pytest.fixture(scope="module")
def spec_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("multistep_spec")
    src, exe = d / "spec.c", d / "spec"
    src.write_text(_MAIN)
    subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src), "-lm"])

    def run(values, mode):
        fin, fout = d / f"{mode}.in", d / f"{mode}.out"
        np.ascontiguousarray(values, dtype=np.float32).tofile(fin)
        subprocess.check_call([str(exe), str(fin), str(fout), mode])
        return np.fromfile(fout, dtype=np.float32)
    return run


def _same_bits(got, want, min_nan):
    both_nan = np.isnan(got) & np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[~both_nan], want.view(np.uint32)[~both_nan])
    assert both_nan.sum() >= min_nan


def test_x0_specification_on_random_and_edge_tuples(spec_program):
    from mixdq_amd.sampler import Schedule
    rng = np.random.default_rng(5)
    rows = Schedule("dpmpp_2m", 6, karras=True).coef
    n = 4096
    t = np.empty((n, 4), dtype=np.float32)
    t[:, 0] = rng.standard_normal(n) * 2
    t[:, 1] = rng.standard_normal(n).astype(np.float16)
    t[:, 2:] = rows[rng.integers(0, 6, n), :2]
    inf = np.float32(np.inf)
    edge = np.array([[0.0, -0.0, 1.0, -1.0], [-0.0, 0.0, 1.0, -1.0], [inf, 1.0, 2.0, -1.0], [inf, inf, 2.0, -1.0],
                     [1.0, -inf, 2.0, -0.5], [3e38, -3e38, 2.0, -2.0], [1e-45, 1e-45, 1.5, -0.5],
                     [np.nan, 1.0, 1.0, -1.0], [1.0, 1.0, 0.0, inf]], dtype=np.float32)
    t = np.concatenate([t, edge])
    got = spec_program(t, "x0")
    want = np.concatenate([M.x0(r[0:1], r[1:2], r[2], r[3]) for r in t])
    assert got.shape == want.shape == (len(t),)
    _same_bits(got, want, 2)


def test_update_2m_specification_on_random_and_edge_tuples(spec_program):
    from mixdq_amd.sampler import Schedule
    rng = np.random.default_rng(6)
    rows = Schedule("dpmpp_2m", 6).coef
    n = 4096
    t = np.empty((n, 6), dtype=np.float32)
    t[:, :3] = rng.standard_normal((n, 3)) * np.array([3.0, 1.0, 1.0])
    t[:, 3:] = rows[rng.integers(1, 5, n)][:, [2, 4, 5]]
    inf = np.float32(np.inf)
    edge = np.array([[0.0, -0.0, 0.0, 1.0, 1.0, -1.0], [-0.0, -0.0, 0.0, 1.0, 1.0, 1.0], [inf, 1.0, 1.0, 0.5, 2.0, -1.0],
                     [inf, inf, 1.0, 0.5, -2.0, -1.0], [1.0, 1.0, np.nan, 0.5, 2.0, -1.0], [1.0, 1.0, inf, 0.5, 2.0, 0.0],
                     [3e38, 3e38, -3e38, 1.0, 1.0, 1.0], [1e-45, 1e-45, 1e-45, 0.5, 0.5, 0.5],
                     [1.0, 2.0 ** -24, -1.0, 1.0, 1.0, 1.0]], dtype=np.float32)
    t = np.concatenate([t, edge])
    got = spec_program(t, "2m")
    want = np.concatenate([M.update_2m(r[0:1], r[1:2], r[2:3], r[3], r[4], r[5]) for r in t])
    _same_bits(got, want, 3)
    # the grouping is ((A x) + (B x0)) + (D h): (1 + 2^-24) - 1 with the sum rounded first is 0, not 2^-24
    assert got[-1] == 0.0


# ---- the C ABI -----------------------------------------------------------------------------------------------------
def _lib():
    from mixdq_amd.build import build
    return ctypes.CDLL(build())


def test_entry_points_are_declared_and_exported():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "mixdq_hip.h")).read()
    for name in ("mixdq_sampler_step_2m", "mixdq_sampler_step_2m_masked"):
        assert hasattr(lib, name), name
        assert f"int {name}(" in header, name
    assert "#define MIXDQ_ABI_VERSION 3" in header
    lib.mixdq_abi_version.restype = ctypes.c_int
    assert lib.mixdq_abi_version() == 3
    math_h = open(os.path.join(ROOT, "include", "mixdq_math.h")).read()
    assert "mixdq_sampler_x0(" in math_h and "mixdq_sampler_update_2m(" in math_h


def test_step_2m_rejects_bad_arguments():
    """Never-dereferenced pointers: every call fails its checks on the host, before any launch."""
    lib = _lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    plain, masked = lib.mixdq_sampler_step_2m, lib.mixdq_sampler_step_2m_masked
    plain.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, ctypes.c_float, i64, i32, i64, vp]
    masked.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, ctypes.c_float, i64, i32, i64, vp, vp, vp, i32, vp, vp]
    plain.restype = masked.restype = i32
    p, q = 0x1000, 0x9000

    def call_plain(x=p, eps=p, inp=p, hist=q, coef=p, tt=p, n_steps=4, step=p, first=p, ts=p, n=64, rows=1, rs=64):
        return plain(x, eps, inp, hist, coef, tt, n_steps, step, first, ts, 0.0, n, rows, rs, None)

    def call_masked(x=p, eps=p, inp=p, hist=q, coef=p, tt=p, n_steps=4, step=p, first=p, ts=p, n=64, rows=1, rs=64,
                    z=p, n0=p, mask=p, channels=4, blend=p):
        return masked(x, eps, inp, hist, coef, tt, n_steps, step, first, ts, 0.0, n, rows, rs, z, n0, mask, channels,
                      blend, None)
    for call in (call_plain, call_masked):
        # the plain step's lines
        for name in ("x", "eps", "inp", "coef", "tt", "step", "ts"):
            assert call(**{name: None}) == INVALID, name
        assert call(rows=3) == INVALID and call(rows=0) == INVALID and call(n=-1) == INVALID
        assert call(n_steps=0) == INVALID and call(rows=2, rs=56) == INVALID
        assert call(x=p + 4) == ALIGNMENT and call(eps=p + 2) == ALIGNMENT and call(inp=p + 8) == ALIGNMENT
        assert call(n=68, rows=2, rs=68) == ALIGNMENT and call(step=p + 2) == ALIGNMENT
        # the new operands
        assert call(hist=None) == INVALID and call(first=None) == INVALID
        assert call(hist=p) == INVALID and call(hist=p + 4 * 63) == INVALID and call(x=q + 16, hist=q) == INVALID
        assert call(hist=q + 4) == ALIGNMENT and call(hist=q + 8) == ALIGNMENT
        assert call(coef=p + 4) == ALIGNMENT and call(coef=p + 8) == ALIGNMENT
        assert call(first=p + 2) == ALIGNMENT and call(first=p + 1) == ALIGNMENT
        assert call(hist=None, first=p + 2) == INVALID      # an invalid argument is named before a misaligned one
    for name in ("z", "n0", "mask", "blend"):
        assert call_masked(**{name: None}) == INVALID, name
    assert call_masked(channels=0) == INVALID and call_masked(n=64, channels=3) == INVALID
    assert call_masked(z=p + 4) == ALIGNMENT and call_masked(n0=p + 8) == ALIGNMENT
    assert call_masked(mask=p + 2) == ALIGNMENT and call_masked(blend=p + 4) == ALIGNMENT
    assert call_masked(z=p + 4, channels=0) == INVALID
