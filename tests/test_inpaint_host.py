"""Inpainting on the host: Schedule.blend against the schedulers' textbook add_noise in float64, the three new entry
points loaded on a CPU-only box (declared, exported, every refusal of their argument checks), and the two new
functions of include/mixdq_math.h -- compiled by the host compiler without contraction into a stand-alone program --
against their numpy restatement (tests/inpaint_ref.py) bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import inpaint_ref as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("euler_ancestral", "euler", "lcm")
OK, INVALID, ALIGNMENT = 0, 1, 2


def _ac():
    betas = np.linspace(np.sqrt(0.00085), np.sqrt(0.012), 1000, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas)


@pytest.mark.parametrize("n_steps", [1, 2, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_blend_table_is_add_noise_at_the_next_timestep(kind, n_steps):
    """Row i < n - 1: add_noise at timesteps[i + 1] -- the Euler schedulers' `original + noise * sigma`, LCM's (DDPM's)
    `sqrt(ac) * original + sqrt(1 - ac) * noise` -- written out in float64 and rounded once to FP32; the last row is
    (1, 0)."""
    from mixdq_amd.sampler import schedule
    s = schedule(kind, n_steps)
    ac = _ac()
    assert s.blend.dtype == np.float32 and s.blend.shape == (n_steps, 2)
    for i in range(n_steps - 1):
        a = ac[s.timesteps[i + 1]]
        want = (np.sqrt(a), np.sqrt(1.0 - a)) if kind == "lcm" else (1.0, np.sqrt((1.0 - a) / a))
        assert s.blend[i].tolist() == [float(np.float32(want[0])), float(np.float32(want[1]))], (kind, n_steps, i)
        assert s.blend[i].tolist() == [float(np.float32(v)) for v in s.start(i + 1)[:2]]
    assert s.blend[-1].tolist() == [1.0, 0.0]
    if n_steps > 1:
        assert (np.diff(s.blend[:, 1]) < 0).all()                 # the kept region's noise level falls step by step


def _lib():
    from mixdq_amd.build import build
    return ctypes.CDLL(build())


def test_entry_points_are_declared_and_exported():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "mixdq_hip.h")).read()
    for name in ("mixdq_sampler_step_masked", "mixdq_mask_to_latent", "mixdq_composite_u8"):
        assert hasattr(lib, name), name
        assert f"int {name}(" in header, name
    for line in ("#define MIXDQ_MASK_NEAREST 0", "#define MIXDQ_MASK_ANY 1", "#define MIXDQ_ABI_VERSION 3"):
        assert line in header
    lib.mixdq_abi_version.restype = ctypes.c_int
    assert lib.mixdq_abi_version() == 3
    math_h = open(os.path.join(ROOT, "include", "mixdq_math.h")).read()
    assert "mixdq_sampler_blend(" in math_h and "mixdq_to_uint8(" in math_h


def test_masked_step_rejects_bad_arguments():
    """Never-dereferenced pointers: every call fails its checks on the host, before any launch."""
    lib = _lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    fn = lib.mixdq_sampler_step_masked
    fn.argtypes = [vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, ctypes.c_float, i64, i32, i64, vp, vp, vp, i32, vp, vp]
    fn.restype = i32
    p = 0x1000

    def call(x=p, eps=p, inp=p, noise=None, ns=0, coef=p, tt=p, n_steps=4, step=p, ts=p, n=64, rows=1, rs=64, z=p,
             n0=p, mask=p, channels=4, blend=p):
        return fn(x, eps, inp, noise, ns, coef, tt, n_steps, step, ts, 0.0, n, rows, rs, z, n0, mask, channels, blend,
                  None)
    # the plain step's lines, unchanged
    assert call(x=None) == INVALID and call(tt=None) == INVALID
    assert call(rows=3) == INVALID and call(rows=0) == INVALID and call(n=-1) == INVALID and call(n_steps=0) == INVALID
    assert call(rows=2, rs=56) == INVALID
    assert call(x=p + 4) == ALIGNMENT and call(eps=p + 2) == ALIGNMENT
    assert call(n=68, rows=2, rs=68) == ALIGNMENT and call(noise=p, ns=66) == ALIGNMENT
    # the new ones
    for name in ("z", "n0", "mask", "blend"):
        assert call(**{name: None}) == INVALID, name
    assert call(channels=0) == INVALID and call(channels=-4) == INVALID
    assert call(n=64, channels=3) == INVALID and call(n=4, channels=8) == INVALID          # n % channels != 0
    assert call(z=p + 4) == ALIGNMENT and call(z=p + 8) == ALIGNMENT
    assert call(n0=p + 4) == ALIGNMENT and call(n0=p + 8) == ALIGNMENT
    assert call(mask=p + 2) == ALIGNMENT and call(mask=p + 1) == ALIGNMENT
    assert call(blend=p + 4) == ALIGNMENT and call(blend=p + 2) == ALIGNMENT
    # an invalid argument is named before a misaligned one, as in the plain step
    assert call(z=p + 4, channels=0) == INVALID


def test_mask_to_latent_rejects_bad_arguments():
    lib = _lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    fn = lib.mixdq_mask_to_latent
    fn.argtypes = [vp, i32, i64, i64, i64, vp, i32, i32, i32, i32, vp]
    fn.restype = i32
    p = 0x1000

    def call(mask=p, dtype=0, out=p, B=1, H=16, W=24, mode=0):
        return fn(mask, dtype, H * W, W, 1, out, B, H, W, mode, None)
    assert call(H=12) == INVALID and call(W=20) == INVALID and call(H=7, W=7) == INVALID
    assert call(dtype=3) == INVALID and call(dtype=-1) == INVALID
    assert call(mode=2) == INVALID and call(mode=-1) == INVALID
    assert call(B=-1) == INVALID
    assert call(mask=None) == INVALID and call(out=None) == INVALID
    assert call(mask=p + 1, dtype=1) == ALIGNMENT and call(mask=p + 2, dtype=2) == ALIGNMENT
    assert call(out=p + 2) == ALIGNMENT
    # nothing to do: no pointer is looked at, nothing is launched
    assert call(mask=None, out=None, B=0) == OK and call(mask=None, out=None, H=0) == OK
    assert call(mask=None, out=None, W=0, mode=1, dtype=2) == OK
    assert call(mask=None, out=None, B=0, mode=5) == INVALID        # ... but the codes are still checked


def test_composite_rejects_bad_arguments():
    lib = _lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    fn = lib.mixdq_composite_u8
    fn.argtypes = [vp] + [i64] * 4 + [vp] + [i64] * 4 + [vp, i32] + [i64] * 3 + [vp, i32, i32, i32, vp]
    fn.restype = i32
    p = 0x1000

    def call(dec=p, orig=p, mask=p, dtype=0, out=p, B=1, H=16, W=24):
        return fn(dec, 4 * H * W, 1, 4 * W, 4, orig, 3 * H * W, H * W, W, 1, mask, dtype, H * W, W, 1, out, B, H, W, None)
    for name in ("dec", "orig", "mask", "out"):
        assert call(**{name: None}) == INVALID, name
    assert call(dtype=3) == INVALID and call(dtype=-1) == INVALID and call(B=-1) == INVALID and call(W=-8) == INVALID
    assert call(dec=p + 1) == ALIGNMENT
    assert call(mask=p + 1, dtype=1) == ALIGNMENT and call(mask=p + 2, dtype=2) == ALIGNMENT
    assert call(dec=None, orig=None, mask=None, out=None, B=0) == OK
    assert call(dec=None, orig=None, mask=None, out=None, H=0) == OK


_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "mixdq_math.h"

/* spec IN OUT u8|blend: IN holds FP32 values (u8: one per result; blend: six per result -- x_new, z, n0, m, p, q) */
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 3;
  if (argv[3][0] == 'u') {
    float v;
    while (fread(&v, 4, 1, in) == 1) {
      const uint8_t u = mixdq_to_uint8(v);
      fwrite(&u, 1, 1, out);
    }
  } else {
    float t[6];
    while (fread(t, 4, 6, in) == 6) {
      const float r = mixdq_sampler_blend(t[0], t[1], t[2], t[3], t[4], t[5]);
      fwrite(&r, 4, 1, out);
    }
  }
  fclose(in);
  return fclose(out) ? 4 : 0;
}
"""


@pytest.fixture(scope="module")
def spec_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("inpaint_spec")
    src, exe = d / "spec.c", d / "spec"
    src.write_text(_MAIN)
    subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src), "-lm"])

    def run(values, mode, dtype):
        fin, fout = d / f"{mode}.in", d / f"{mode}.out"
        np.ascontiguousarray(values, dtype=np.float32).tofile(fin)
        subprocess.check_call([str(exe), str(fin), str(fout), mode])
        return np.fromfile(fout, dtype=dtype)
    return run


def test_to_uint8_specification_on_every_fp16_pattern(spec_program):
    """mixdq_to_uint8 == the restatement for all 65 536 FP16 bit patterns (NaNs, infinities, subnormals, the ties of
    the rounding), and == the formula in float64 with round-half-even wherever that is further than 1e-4 from a tie:
    the FP32 sum is off by at most 2^-25 (255 * 2^-25 = 7.6e-6 after the product) and the product by at most
    255 * 2^-24 = 1.5e-5, so off the ties both round to the same integer."""
    halves = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    got = spec_program(halves.astype(np.float32), "u8", np.uint8)
    want = I.to_uint8(halves)
    assert got.shape == want.shape == (65536,)
    assert np.array_equal(got, want), f"{int((got != want).sum())} patterns differ"
    nan = np.isnan(halves)
    assert nan.sum() == 2046 and (got[nan] == 0).all()                           # NaN is 0
    assert got[halves == np.inf][0] == 255 and got[halves == -np.inf][0] == 0
    fin = ~nan & np.isfinite(halves)
    exact = np.clip(halves[fin].astype(np.float64) / 2 + 0.5, 0.0, 1.0) * 255.0
    off_tie = np.abs(exact - np.floor(exact) - 0.5) > 1e-4
    assert np.array_equal(got[fin][off_tie], np.rint(exact[off_tie]).astype(np.uint8))
    assert got[halves == np.float16(1.0)][0] == 255 and got[halves == np.float16(-1.0)][0] == 0
    assert got[halves == np.float16(0.0)][0] == 128                             # 127.5 exactly: half to even


def test_blend_specification_on_random_and_edge_tuples(spec_program):
    rng = np.random.default_rng(77)
    n = 4096
    t = np.empty((n, 6), dtype=np.float32)
    t[:, :3] = rng.standard_normal((n, 3)) * np.array([3.0, 0.2, 1.0])
    t[:, 3] = rng.choice(np.array([0.0, 1.0, 0.25], dtype=np.float32), n)
    t[:, 4] = rng.choice(np.array([1.0, 0.9983, 0.31], dtype=np.float32), n)
    t[:, 5] = rng.choice(np.array([0.0, 14.6, 0.058, 0.95], dtype=np.float32), n)
    t[:512, 3] = rng.random(512)                                                # soft masks
    inf = np.float32(np.inf)
    edge = np.array([[0.0, -0.0, 0.0, 0.0, 1.0, 0.0], [-0.0, -0.0, -0.0, 1.0, 1.0, 0.0],
                     [-0.0, 0.0, 0.0, 1.0, 1.0, 0.0], [1.5, -0.0, -0.0, 0.0, 1.0, 1.0],
                     [inf, 1.0, 1.0, 0.0, 1.0, 0.5], [inf, 1.0, 1.0, 1.0, 1.0, 0.5], [-inf, 1.0, 1.0, 0.25, 1.0, 0.5],
                     [1.0, inf, 1.0, 1.0, 1.0, 0.5], [1.0, inf, 1.0, 0.0, 1.0, 0.5], [1.0, 2.0, -inf, 0.0, 1.0, 0.0],
                     [1.0, inf, -inf, 0.25, 1.0, 1.0], [3e38, 3e38, 3e38, 0.25, 1.0, 1.0],
                     [1e-45, 1e-45, 1e-45, 0.25, 1.0, 1.0]], dtype=np.float32)
    t = np.concatenate([t, edge])
    got = spec_program(t, "blend", np.float32)
    want = np.empty(len(t), dtype=np.float32)
    for p in np.unique(t[:, 4]):
        for q in np.unique(t[:, 5]):
            sel = (t[:, 4] == p) & (t[:, 5] == q)
            if sel.any():
                want[sel] = I.blend(t[sel, 0], t[sel, 1], t[sel, 2], t[sel, 3], p, q)
    both_nan = np.isnan(got) & np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[~both_nan], want.view(np.uint32)[~both_nan])
    assert both_nan.sum() >= 3                                                   # 0 * inf, inf - inf
    # m == 0 gives k and m == 1 gives x_new, up to the sign of zero, wherever everything is finite
    finite = np.isfinite(t).all(axis=1)
    keep, paint = finite & (t[:, 3] == 0), finite & (t[:, 3] == 1)
    assert keep.sum() > 1000 and paint.sum() > 1000
    for sel in (keep,):
        k = np.array([I.kept(z, n0, p, q) for z, n0, p, q in t[sel][:, [1, 2, 4, 5]]], dtype=np.float32)
        assert np.array_equal(got[sel], k)                                       # (== : -0 equals +0)
    assert np.array_equal(got[paint], t[paint, 0])
