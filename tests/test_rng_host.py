"""The device-side noise on the host (no GPU): Philox4x32-10 against the Random123 known answers, the functions of
include/mixdq_math.h -- compiled by the host compiler without contraction into a stand-alone program -- against their
numpy restatement (tests/rng_ref.py) bit for bit, the accuracy of the restatement's log / sin / cos against float64 over
ALL 2^24 arguments, the distribution of what the counter layout produces, and the declarations and argument checks of
the new entry points and bindings."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import rng_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, ALIGNMENT = 0, 1, 2
LOG_ULP, SINCOS_ULP = 0.851, 1.015       # the bounds include/mixdq_math.h states (the issue's ceiling: 2)
KAT = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        "d16cfe09 94fdcceb 5001e420 24126ea1"))

_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "mixdq_math.h"

/* spec IN OUT MODE: IN holds uint32 tuples --
 *   philox: (c0, c1, c2, c3, k0, k1) -> four uint32        bits:   (r0, r1, r2, r3) -> four FP32 (mixdq_rng_normals4)
 *   log:    (k) -> one FP32                                 sincos: (j) -> (sin, cos)
 *   at:     (seed lo, seed hi, e lo, e hi, step, stream) -> one FP32 (mixdq_rng_normal_at)
 *   image:  (seed lo, seed hi, n lo, n hi, step, stream) -> n FP32, whole calls (mixdq_rng_quad), the last one cut */
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 3;
  uint32_t t[6];
  const char m = argv[3][0];
  if (m == 'p') {
    while (fread(t, 4, 6, in) == 6) {
      uint32_t r[4];
      mixdq_philox4x32_10(t, t + 4, r);
      fwrite(r, 4, 4, out);
    }
  } else if (m == 'b') {
    while (fread(t, 4, 4, in) == 4) {
      float z[4];
      mixdq_rng_normals4(t, z);
      fwrite(z, 4, 4, out);
    }
  } else if (m == 'l') {
    while (fread(t, 4, 1, in) == 1) {
      const float r = mixdq_rng_log_u24(t[0]);
      fwrite(&r, 4, 1, out);
    }
  } else if (m == 's') {
    while (fread(t, 4, 1, in) == 1) {
      float sc[2];
      mixdq_rng_sincos_u24(t[0], &sc[0], &sc[1]);
      fwrite(sc, 4, 2, out);
    }
  } else if (m == 'a') {
    while (fread(t, 4, 6, in) == 6) {
      const float r = mixdq_rng_normal_at(t[0] | ((uint64_t)t[1] << 32), t[2] | ((uint64_t)t[3] << 32), t[4], t[5]);
      fwrite(&r, 4, 1, out);
    }
  } else {
    while (fread(t, 4, 6, in) == 6) {
      const uint64_t seed = t[0] | ((uint64_t)t[1] << 32), n = t[2] | ((uint64_t)t[3] << 32);
      for (uint64_t q = 0; 4 * q < n; ++q) {
        float z[4];
        mixdq_rng_quad(seed, q, t[4], t[5], z);
        fwrite(z, 4, n - 4 * q < 4 ? n - 4 * q : 4, out);
      }
    }
  }
  fclose(in);
  return fclose(out) ? 4 : 0;
}
"""


@pytest.fixture(scope="module")
def spec_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("rng_spec")
    src, exe = d / "spec.c", d / "spec"
    src.write_text(_MAIN)
    subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src), "-lm"])
    count = itertools.count()

    def run(words, mode, dtype=np.float32):
        i = next(count)
        fin, fout = d / f"{i}.in", d / f"{i}.out"
        np.ascontiguousarray(words, dtype=np.uint32).tofile(fin)
        subprocess.check_call([str(exe), str(fin), str(fout), mode])
        got = np.fromfile(fout, dtype=dtype)
        os.remove(fin)
        os.remove(fout)
        return got
    return run


def _image_words(seed, n, step, stream):
    return [seed & 0xffffffff, seed >> 32, n & 0xffffffff, n >> 32, step, stream]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- Philox ----------------------------------------------------------------------------------------------------------
def test_philox_known_answers(spec_program):
    for ctr, key, want in KAT:
        ref = " ".join("%08x" % int(v) for v in R.philox4x32_10(ctr, key))
        got = " ".join("%08x" % int(v) for v in spec_program(list(ctr) + list(key), "philox", np.uint32))
        assert ref == want and got == want, (ctr, key, ref, got)
    rng = np.random.default_rng(1)
    words = rng.integers(0, 2 ** 32, (4096, 6), dtype=np.uint64).astype(np.uint32)
    got = spec_program(words, "philox", np.uint32).reshape(-1, 4)
    want = np.stack(R.philox4x32_10(words[:, :4].T, words[:, 4:].T), axis=1)
    assert np.array_equal(got, want)
    # a vectorised call of the restatement is its scalar call
    assert [int(v[0]) for v in R.philox4x32_10([[c] for c in KAT[2][0]], [[k] for k in KAT[2][1]])] == \
        [int(w, 16) for w in KAT[2][2].split()]


# ---- the map from words to normals ---------------------------------------------------------------------------------
def _octant_edges():
    j = []
    for o in range(9):
        for d in (-2, -1, 0, 1, 2):
            v = o * (1 << 21) + d
            if 0 <= v < (1 << 24):
                j.append(v)
    return np.array(sorted(set(j)), dtype=np.uint32)


def test_normals_from_bits_on_random_and_edge_words(spec_program):
    """Compiled header == numpy restatement, bit for bit: r0 >> 8 in {0, 1, 2^24 - 1} (u1 = 2^-24: the largest radius;
    u1 = 1: radius 0), r1 >> 8 on and beside every octant boundary, the low 8 bits (which must not matter) set and clear,
    and random words."""
    rng = np.random.default_rng(2)
    words = [rng.integers(0, 2 ** 32, (1 << 16, 4), dtype=np.uint64).astype(np.uint32)]
    edges = _octant_edges()
    for k0 in (0, 1, (1 << 24) - 1, 0x800000, 0x5a5a5a):
        for low in (0, 0xff):
            w = np.empty((len(edges), 4), dtype=np.uint32)
            w[:, 0] = (k0 << 8) | low
            w[:, 1] = (edges << np.uint32(8)) | np.uint32(low)
            w[:, 2] = w[:, 1][::-1]                                   # the second pair takes the same care
            w[:, 3] = w[:, 0]
            words.append(w)
    words = np.concatenate(words)
    got = spec_program(words, "bits").reshape(-1, 4)
    want = R.normals_from_bits(words)
    assert np.isfinite(want).all() and np.abs(want).max() <= 5.78
    assert np.array_equal(_bits(got), _bits(want))
    # the low byte of a word is not used
    assert np.array_equal(_bits(R.normals_from_bits(words | np.uint32(0xff))),
                          _bits(R.normals_from_bits(words & np.uint32(0xffffff00))))
    # the largest radius: u1 = 2^-24, sqrt(48 ln 2); along the axis (u2 = 0) z0 is that radius and z1 is 0
    z = R.normals_from_bits(np.array([[0, 0, 0xffffffff, 0x40000000]], dtype=np.uint32))[0]
    assert abs(float(z[0]) - np.sqrt(48 * np.log(2.0))) < 1e-6 and z[1] == 0.0
    assert z[2] == 0.0 and z[3] == 0.0                                # u1 = 1: radius 0


def test_element_rule_matches_whole_calls(spec_program):
    """mixdq_rng_normal_at (one element alone) and mixdq_rng_quad (a whole call) are the same values, and both are the
    restatement's image: seeds with a high word, steps and streams in the counter's upper words, n_image % 4 != 0."""
    for seed, n, step, stream in ((0, 37, 0, 0), (0x0123456789abcdef, 64, 7, 1), (2 ** 64 - 1, 4099, 1, 1),
                                  (1 << 32, 1, 0, 2), (5, 2, 3, 1)):
        want = R.randn_image(seed, n, stream, step)
        img = spec_program([_image_words(seed, n, step, stream)], "image")
        at = spec_program([[seed & 0xffffffff, seed >> 32, e, 0, step, stream] for e in range(n)], "at")
        assert want.shape == (n,) and np.array_equal(_bits(img), _bits(want)) and np.array_equal(_bits(at), _bits(want))
    # elements past 2^34: the counter's second word (the restatement's quad index is 64-bit as well)
    e = (1 << 34) + 5
    at = spec_program([[9, 0, e & 0xffffffff, e >> 32, 0, 0]], "at")
    r = R.philox4x32_10((np.uint32((e >> 2) & 0xffffffff), np.uint32(e >> 34), 0, 0), (9, 0))
    assert _bits(at)[0] == _bits(R.normals_from_bits(np.array([[int(v) for v in r]], dtype=np.uint32)))[0, e & 3]
    # what differs: seed, step, stream each change the values
    base = R.randn_image(3, 64)
    for other in (R.randn_image(4, 64), R.randn_image(3, 64, stream=1), R.randn_image(3, 64, step=1),
                  R.randn_image(3 + (1 << 32), 64)):
        assert not np.array_equal(base, other)
    # what does not: the image's length (a longer image starts with the shorter one's values)
    assert np.array_equal(R.randn_image(3, 61), base[:61])
    got = R.randn((2, 3, 2, 5), [3, 4])
    assert got.shape == (2, 3, 2, 5) and np.array_equal(got[0].transpose(1, 2, 0).reshape(-1), R.randn_image(3, 30))


# ---- accuracy over all 2^24 arguments ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exhaustive():
    k = np.arange(1, (1 << 24) + 1, dtype=np.uint32)
    j = np.arange(1 << 24, dtype=np.uint32)
    return {"k": k, "j": j, "log": R.log_u24(k), "sincos": R.sincos_u24(j)}


def test_log_accuracy_over_all_arguments(exhaustive, spec_program):
    k, lg = exhaustive["k"], exhaustive["log"]
    exact = np.log(k.astype(np.float64)) - 24.0 * np.log(2.0)
    err = R.ulp_error(lg, exact)
    print(f"log: max {err.max():.4f} ulp at k = {int(k[err.argmax()])}")
    assert err.max() <= LOG_ULP <= 2.0
    assert lg[-1] == 0.0 and (lg <= 0).all() and np.isfinite(lg).all()        # sqrt(-2 log) never sees a negative
    assert np.array_equal(_bits(spec_program(k, "log")), _bits(lg))           # the compiled header, all 2^24


def test_sincos_accuracy_over_all_arguments(exhaustive, spec_program):
    j = exhaustive["j"]
    sn, cs = exhaustive["sincos"]
    # float64 reference through the same exact reduction (so that it is accurate next to the zeros)
    octant = j >> 21
    r = (j & 0x1fffff).astype(np.float64)
    x = np.where(octant & 1, (1 << 21) - r, r) * (np.pi / 4 / (1 << 21))
    s_, c_ = np.sin(x), np.cos(x)
    swap = ((octant + 1) >> 1) & 1
    exact_s = np.where(swap, c_, s_) * np.where(octant >= 4, -1.0, 1.0)
    exact_c = np.where(swap, s_, c_) * np.where(((octant + 2) >> 2) & 1, -1.0, 1.0)
    ang = j.astype(np.float64) * (2 * np.pi / (1 << 24))
    assert np.abs(exact_s - np.sin(ang)).max() < 1e-15 and np.abs(exact_c - np.cos(ang)).max() < 1e-15
    es, ec = R.ulp_error(sn, exact_s), R.ulp_error(cs, exact_c)
    print(f"sin: max {es.max():.4f} ulp at j = {int(j[es.argmax()])}; cos: max {ec.max():.4f} ulp at j = {int(j[ec.argmax()])}")
    assert es.max() <= SINCOS_ULP <= 2.0 and ec.max() <= SINCOS_ULP
    assert (np.abs(sn) <= 1).all() and (np.abs(cs) <= 1).all()
    got = spec_program(j, "sincos").reshape(-1, 2)
    assert np.array_equal(_bits(got[:, 0]), _bits(sn)) and np.array_equal(_bits(got[:, 1]), _bits(cs))


def test_header_states_the_measured_bounds():
    math_h = open(os.path.join(ROOT, "include", "mixdq_math.h")).read()
    assert f"max error {LOG_ULP} ulp over all 2^24 arguments" in math_h
    assert f"max error {SINCOS_ULP} ulp over all 2^24 arguments" in math_h
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert str(LOG_ULP) in design and str(SINCOS_ULP) in design


# ---- distribution --------------------------------------------------------------------------------------------------
N = 1 << 20
SEEDS = (0, 1, 0x0123456789abcdef, 2 ** 64 - 1)
COUNTERS = ((0, 0), (0, 1), (1, 1), (7, 1), (0, 2))          # (step, stream)
CASES = [(s, c) for s in SEEDS for c in COUNTERS]


@pytest.fixture(scope="module")
def samples(spec_program):
    """The 20 cases, 2^20 normals each, float64 [20, N]: generated by the compiled header (the restatement would take
    a minute); one case is checked against the restatement in full, every case over its first 4096 elements."""
    z = np.stack([spec_program([_image_words(seed, N, step, stream)], "image") for seed, (step, stream) in CASES])
    assert z.shape == (len(CASES), N)
    for i, (seed, (step, stream)) in enumerate(CASES):
        n = N if i == 13 else 4096
        assert np.array_equal(_bits(z[i, :n]), _bits(R.randn_image(seed, n, stream, step)))
    return z.astype(np.float64)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_distribution(samples, case):
    import torch
    z = samples[case]
    mean, var = z.mean(), z.var()
    m4 = ((z - mean) ** 4).mean() / var ** 2
    zs = np.sort(z)
    cdf = (0.5 * (1.0 + torch.erf(torch.from_numpy(zs) / np.sqrt(2.0)))).numpy()
    i = np.arange(N, dtype=np.float64)
    ks = max(np.abs(cdf - i / N).max(), np.abs(cdf - (i + 1) / N).max())
    lag = max(abs(float(np.mean(z[:-k] * z[k:]))) for k in range(1, 9))
    print(f"case {CASES[case]}: mean {mean * np.sqrt(N):+.2f} sigma, var {(var - 1) / np.sqrt(2 / N):+.2f} sigma, "
          f"m4 {(m4 - 3) / np.sqrt(96 / N):+.2f} sigma, KS*sqrt(N) {ks * np.sqrt(N):.3f}, max|z| {np.abs(z).max():.3f}, "
          f"lag 1..8 autocorrelation <= {lag * np.sqrt(N):.2f} sigma")
    assert abs(mean) < 4 / np.sqrt(N)
    assert abs(var - 1) < 4 * np.sqrt(2 / N)
    assert abs(m4 - 3) < 4 * np.sqrt(96 / N)
    assert ks < 1.95 / np.sqrt(N)
    assert np.abs(z).max() <= 5.78


def test_cases_are_uncorrelated(samples):
    g = samples @ samples.T / N
    pairs = [(a, b) for a in range(len(CASES)) for b in range(a + 1, len(CASES))]
    assert len(pairs) == 190
    worst = max(abs(g[a, b]) for a, b in pairs)
    print(f"pairwise correlation: worst {worst * np.sqrt(N):.2f} sigma over {len(pairs)} pairs")
    assert worst < 5 / np.sqrt(N)


# ---- declarations and binding ----------------------------------------------------------------------------------------
NEW = ("mixdq_randn_f32", "mixdq_rng_normals_from_bits", "mixdq_sampler_step_rng", "mixdq_sampler_step_masked_rng")


def _lib():
    from mixdq_amd.build import build
    return ctypes.CDLL(build())


def test_entry_points_are_declared_and_exported():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "mixdq_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert f"int {name}(" in header, name
    for i, name in enumerate(("START", "STEP", "VAE")):
        assert f"#define MIXDQ_RNG_STREAM_{name} {i}" in header
    assert "#define MIXDQ_ABI_VERSION 3" in header
    lib.mixdq_abi_version.restype = ctypes.c_int
    assert lib.mixdq_abi_version() == 3
    math_h = open(os.path.join(ROOT, "include", "mixdq_math.h")).read()
    for name in ("mixdq_philox4x32_10(", "mixdq_rng_log_u24(", "mixdq_rng_sincos_u24(", "mixdq_rng_normals4(",
                 "mixdq_rng_normal_at("):
        assert name in math_h, name
    from mixdq_amd import _C
    assert (_C.RNG_STREAM_START, _C.RNG_STREAM_STEP, _C.RNG_STREAM_VAE) == (0, 1, 2) == \
        (R.STREAM_START, R.STREAM_STEP, R.STREAM_VAE)
    assert _C.EXPECTED_ABI == 3


def test_entry_points_reject_bad_arguments():
    """Never-dereferenced pointers: every call fails its checks on the host, before any launch."""
    lib = _lib()
    vp, i64, i32, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32
    randn, bits = lib.mixdq_randn_f32, lib.mixdq_rng_normals_from_bits
    plain, masked = lib.mixdq_sampler_step_rng, lib.mixdq_sampler_step_masked_rng
    randn.argtypes = [vp, i32, i64, vp, u32, u32, vp]
    bits.argtypes = [vp, vp, i64, vp]
    plain.argtypes = [vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, ctypes.c_float, i64, i32, i64, vp]
    masked.argtypes = plain.argtypes[:-1] + [vp, vp, vp, i32, vp, vp]
    for f in (randn, bits, plain, masked):
        f.restype = i32
    p = 0x1000
    assert randn(None, 1, 8, p, 0, 0, None) == INVALID and randn(p, 1, 8, None, 0, 0, None) == INVALID
    assert randn(p, -1, 8, p, 0, 0, None) == INVALID and randn(p, 1, 0, p, 0, 0, None) == INVALID
    assert randn(p + 4, 1, 8, p, 0, 0, None) == ALIGNMENT and randn(p, 1, 8, p + 4, 0, 0, None) == ALIGNMENT
    assert randn(p + 2, 1, 7, p, 0, 0, None) == ALIGNMENT
    assert randn(p, 0, 8, p, 0, 0, None) == OK and randn(p + 4, 0, 7, p, 0, 0, None) == OK      # B == 0: nothing to do
    assert bits(None, p, 4, None) == INVALID and bits(p, None, 4, None) == INVALID and bits(p, p, -1, None) == INVALID
    assert bits(p + 4, p, 4, None) == ALIGNMENT and bits(p, p + 8, 4, None) == ALIGNMENT and bits(p, p, 0, None) == OK

    def call_plain(x=p, eps=p, inp=p, seeds=p, n_image=64, coef=p, tt=p, n_steps=4, step=p, ts=p, n=64, rows=1, rs=64):
        return plain(x, eps, inp, seeds, n_image, coef, tt, n_steps, step, ts, 0.0, n, rows, rs, None)

    def call_masked(x=p, eps=p, inp=p, seeds=p, n_image=64, coef=p, tt=p, n_steps=4, step=p, ts=p, n=64, rows=1, rs=64,
                    z=p, n0=p, mask=p, channels=4, blend=p):
        return masked(x, eps, inp, seeds, n_image, coef, tt, n_steps, step, ts, 0.0, n, rows, rs, z, n0, mask, channels,
                      blend, None)
    for call in (call_plain, call_masked):
        for name in ("x", "eps", "inp", "coef", "tt", "step", "ts"):             # the sibling's lines
            assert call(**{name: None}) == INVALID, name
        assert call(rows=3) == INVALID and call(n=-1) == INVALID and call(n_steps=0) == INVALID
        assert call(rows=2, rs=56) == INVALID
        assert call(x=p + 4) == ALIGNMENT and call(eps=p + 2) == ALIGNMENT and call(coef=p + 4) == ALIGNMENT
        assert call(seeds=None) == INVALID and call(n_image=0) == INVALID and call(n_image=-64) == INVALID
        assert call(n_image=48) == INVALID and call(n=128, n_image=96, rs=128) == INVALID          # n % n_image != 0
        assert call(seeds=p + 4) == ALIGNMENT and call(seeds=p + 2) == ALIGNMENT
        assert call(seeds=None, x=p + 4) == ALIGNMENT          # the sibling's checks come first, as a whole
    for name in ("z", "n0", "mask", "blend"):
        assert call_masked(**{name: None}) == INVALID, name
    assert call_masked(channels=0) == INVALID and call_masked(channels=3) == INVALID
    assert call_masked(z=p + 4) == ALIGNMENT and call_masked(blend=p + 4) == ALIGNMENT


def test_bindings_reject_bad_seeds():
    """The `seeds=` checks of the step bindings and randn's come before anything that needs a device."""
    import torch
    from mixdq_amd import _C
    x = torch.zeros(64)
    h = torch.zeros(64, dtype=torch.float16)
    coef, tt = torch.zeros(4, 4), torch.zeros(5)
    step, ts = torch.zeros(1, dtype=torch.int32), torch.zeros(())
    blend = torch.zeros(4, 2)
    seeds = torch.zeros(2, dtype=torch.int64)

    def plain(**kw):
        noise = kw.pop("noise", None)
        _C.sampler_step(x, h, h, coef, tt, step, ts, 0.0, 1, noise, **kw)

    def masked(**kw):
        noise = kw.pop("noise", None)
        _C.sampler_step_masked(x, h, h, coef, tt, step, ts, x, x, x, blend, 0.0, 1, noise, **kw)
    for call in (plain, masked):
        with pytest.raises(RuntimeError, match="noise and seeds exclude"):
            call(noise=torch.zeros(4, 64), seeds=seeds, n_image=32)
        with pytest.raises(RuntimeError, match=r"int64 tensor of shape \[2\]"):
            call(seeds=seeds.to(torch.int32), n_image=32)
        with pytest.raises(RuntimeError, match=r"int64 tensor of shape \[2\]"):
            call(seeds=torch.zeros(3, dtype=torch.int64), n_image=32)
        with pytest.raises(RuntimeError, match=r"int64 tensor of shape \[2\]"):
            call(seeds=torch.zeros(2, 1, dtype=torch.int64), n_image=32)
        with pytest.raises(RuntimeError, match=r"int64 tensor of shape \[1\]"):
            call(seeds=seeds)                                         # n_image defaults to n: one image
        with pytest.raises(RuntimeError, match=r"int64 tensor of shape \[2\]"):
            call(seeds=[1, 2], n_image=32)
        with pytest.raises(RuntimeError, match="not a multiple of n_image"):
            call(seeds=seeds, n_image=48)
        with pytest.raises(RuntimeError, match="not a multiple of n_image"):
            call(seeds=seeds, n_image=0)
        with pytest.raises(RuntimeError, match="on x's GPU"):         # well-formed seeds: on to the device checks
            call(seeds=seeds, n_image=32)
    with pytest.raises(RuntimeError, match=r"int64 tensor of shape \[3\]"):
        _C.randn((3, 4, 2, 2), seeds)
    with pytest.raises(RuntimeError, match=r"int64 tensor of shape \[2\]"):
        _C.randn((2, 4, 2, 2), seeds.to(torch.float32))
    with pytest.raises(RuntimeError, match="shape should be"):
        _C.randn((2, 4, 2), seeds)
    with pytest.raises(RuntimeError, match="on the GPU"):
        _C.randn((2, 4, 2, 2), seeds)


def test_seed_tensor_forms():
    import torch
    from mixdq_amd.sampler import seed_tensor
    assert seed_tensor(5, 3, "cpu").tolist() == [5, 6, 7]
    assert seed_tensor(2 ** 64 - 1, 2, "cpu").tolist() == [-1, 0]                 # mod 2^64, bits read as unsigned
    assert seed_tensor(2 ** 63, 1, "cpu").tolist() == [-2 ** 63]
    assert seed_tensor([7, 2 ** 64 - 2], 2, "cpu").tolist() == [7, -2]
    t = torch.tensor([1, -1], dtype=torch.int64)
    assert seed_tensor(t, 2, "cpu") is t
    for bad in (-1, 2 ** 64, [1], [1, -2], [1, 2.0], 1.5, t.to(torch.int32), t[:1]):
        with pytest.raises((RuntimeError, TypeError)):
            seed_tensor(bad, 2, "cpu")
