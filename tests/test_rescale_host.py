"""Guidance rescale on the host (no GPU): the accuracy of the specified summation rule against float64, the functions
of include/mixdq_math.h -- compiled by the host compiler without contraction into a stand-alone program that arranges
the chunk sums as the kernel does -- against tests/rescale_ref.py bit for bit, the defined degenerate cases, and the
Python surface's refusals."""
import os
import subprocess

import numpy as np
import pytest

from tests import multistep_ref as M
from tests import rescale_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _pair(mu, n, seed):
    """(t, e): FP16-rounded N(mu, 1) as the text-conditioned output, and the guided output of it and a second such draw
    at guidance 7.5 -- FP32 values, as the kernel sees them."""
    rng = np.random.default_rng(seed)
    u = (rng.standard_normal(n) + mu).astype(np.float16)
    c = (rng.standard_normal(n) + mu).astype(np.float16)
    return c.astype(f32), M.guided(u, c, 7.5)


def _naive_m2(v):
    """The rule that was NOT chosen, in float32: n * (E[x^2] - mean^2)."""
    v = v.astype(f32)
    n = f32(v.size)
    mean = v.sum(dtype=f32) / n
    return ((v * v).sum(dtype=f32) / n - mean * mean) * n


# ---- accuracy of the specification ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_image", [252, 2072, 16384, 65536])
@pytest.mark.parametrize("mu", [0, 64, 1000])
def test_specification_accuracy(mu, n_image):
    """s = sqrt(M2_t / M2_e) by the chunked rule in float32, in its fixed order, against float64 std(ddof=1) of the same
    values: within 1e-5 relative.  Measured: at most 8.6e-8 over the twelve inputs.  The float32 E[x^2] - mean^2 is
    printed beside it (it is what the bound separates: 2.6e-5 .. 2.9e-4 at mu = 64, 1.8 .. 7.6 % at mu = 1000)."""
    t, e = _pair(mu, n_image, 1000 * mu + n_image)
    want = np.std(t.astype(np.float64), ddof=1) / np.std(e.astype(np.float64), ddof=1)
    got = float(RR.std_ratio(t, e))
    err = abs(got - want) / want
    with np.errstate(invalid="ignore"):
        naive = float(np.sqrt(_naive_m2(t) / _naive_m2(e)))
    print(f"mu {mu} n_image {n_image}: chunked {err:.3e}, float32 E[x^2] - mean^2 {abs(naive - want) / want:.3e}")
    assert err <= 1e-5


# ---- the header is the restatement ---------------------------------------------------------------------------------
_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "mixdq_math.h"

/* S of the specification over 2048 values (absent ones already +0) */
static float ordered_sum(const float* v) {
  float p[256];
  for (int l = 0; l < 256; ++l) p[l] = mixdq_rescale_lane_sum(v + 8 * l);
  for (int k = 1; k < 64; k <<= 1) {
    float q[256];
    for (int l = 0; l < 256; ++l) q[l] = p[l] + p[l ^ k];
    for (int l = 0; l < 256; ++l) p[l] = q[l];
  }
  return ((p[0] + p[64]) + p[128]) + p[192];
}

static void image_stats(const float* v, long n, float* mean, float* m2) {
  *mean = 0.0f, *m2 = 0.0f;
  for (long at = 0; at < n; at += MIXDQ_RESCALE_CHUNK) {
    const long k = n - at < MIXDQ_RESCALE_CHUNK ? n - at : MIXDQ_RESCALE_CHUNK;
    float a[MIXDQ_RESCALE_CHUNK];
    for (long i = 0; i < MIXDQ_RESCALE_CHUNK; ++i) a[i] = i < k ? v[at + i] : 0.0f;
    const float mean_c = ordered_sum(a) / (float)k;
    for (long i = 0; i < MIXDQ_RESCALE_CHUNK; ++i) a[i] = i < k ? mixdq_rescale_sqdev(v[at + i], mean_c) : 0.0f;
    mixdq_rescale_combine(at, k, mean_c, ordered_sum(a), mean, m2);
  }
}

/* spec IN OUT n_image phi: IN holds images of (t[n_image], e[n_image]) FP32; OUT per image (mean_t, M2_t, mean_e, M2_e,
 * r, e[0] * r) */
int main(int argc, char** argv) {
  if (argc != 5) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  const long n = atol(argv[3]);
  const float phi = (float)atof(argv[4]);
  if (!in || !out || n < 1) return 3;
  float* t = (float*)malloc(sizeof(float) * n);
  float* e = (float*)malloc(sizeof(float) * n);
  while (fread(t, 4, n, in) == (size_t)n && fread(e, 4, n, in) == (size_t)n) {
    float r[6];
    image_stats(t, n, &r[0], &r[1]);
    image_stats(e, n, &r[2], &r[3]);
    r[4] = mixdq_rescale_factor(r[1], r[3], phi, n);
    r[5] = mixdq_sampler_rescaled(e[0], r[4]);
    fwrite(r, 4, 6, out);
  }
  free(t), free(e);
  fclose(in);
  return fclose(out) ? 4 : 0;
}
"""


@pytest.fixture(scope="module")
def spec_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("rescale_spec")
    src, exe = d / "spec.c", d / "spec"
    src.write_text(_MAIN)
    subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src), "-lm"])

    def run(images, n_image, phi):
        fin, fout = d / "spec.in", d / "spec.out"
        np.ascontiguousarray(images, dtype=f32).tofile(fin)
        subprocess.check_call([str(exe), str(fin), str(fout), str(n_image), repr(float(phi))])
        return np.fromfile(fout, dtype=f32).reshape(-1, 6)
    return run


@pytest.mark.parametrize("n_image", [1, 7, 252, 2048, 2049, 2072, 6400, 65536])
def test_header_equals_the_restatement(spec_program, n_image):
    images = [_pair(mu, n_image, 7 * n_image + mu) for mu in (0, 64, -3)]
    images.append((np.full(n_image, 2.5, f32), np.full(n_image, 2.5, f32)))          # both spreads zero
    images.append((images[0][0], np.full(n_image, -1.0, f32)))                         # the guided spread zero
    phi = 0.7
    got = spec_program(np.stack([np.stack(p) for p in images]), n_image, phi)
    for (t, e), g in zip(images, got):
        ct, ce = RR.chunk_stats(t), RR.chunk_stats(e)
        (mean_t, m2_t), (mean_e, m2_e) = RR.combine(*ct), RR.combine(*ce)
        r = RR.factor(m2_t, m2_e, phi, n_image)
        want = np.array([mean_t, m2_t, mean_e, m2_e, r, f32(e[0]) * r], dtype=f32)
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (n_image, g, want)
    assert got[3, 4] == 1.0 and got[4, 4] == 1.0
    if n_image > 1:
        assert got[0, 4] != 1.0 and got[1, 4] != 1.0
    else:
        assert (got[:, 4] == 1.0).all()


# ---- the defined cases ---------------------------------------------------------------------------------------------
def test_factor_definitions():
    assert RR.factor(f32(3.0), f32(3.0), 0.7, 100) == 1.0                   # s == 1: exactly 1, whatever phi
    assert RR.factor(f32(0.0), f32(3.0), 0.7, 100) == 1.0
    assert RR.factor(f32(3.0), f32(0.0), 0.7, 100) == 1.0
    assert RR.factor(f32(3.0), f32(12.0), 0.7, 1) == 1.0
    assert RR.factor(f32(3.0), f32(12.0), 0.0, 100) == 1.0                  # phi == 0: the plain step
    assert RR.factor(f32(3.0), f32(12.0), 1.0, 100) == 0.5                  # phi == 1: std(t) / std(e)
    assert RR.factor(f32(3.0), f32(12.0), 0.5, 100) == 0.75
    # diffusers' expression agrees to rounding
    t, e = _pair(0, 16384, 4)
    s = np.std(t.astype(np.float64), ddof=1) / np.std(e.astype(np.float64), ddof=1)
    _, r = RR.rescaled((np.zeros(16384, np.float16), t.astype(np.float16)), 1.0, 0.0, 0.7, 16384)
    assert r[0] == 1.0                                                      # guidance 1: e == t
    rows = _pair(0, 16384, 4)
    got = RR.factor(RR.image_m2(rows[0]), RR.image_m2(rows[1]), 0.7, 16384)
    assert abs(float(got) - (0.7 * s + 0.3)) <= 1e-6


def test_python_surface_refuses():
    from mixdq_amd.sampler import Sampler
    with pytest.raises(ValueError, match="guidance_rescale"):
        Sampler(None, "euler", 4, guidance_scale=0.0, guidance_rescale=0.7)       # one row per image
    with pytest.raises(ValueError, match="guidance_rescale"):
        Sampler(None, "euler", 4, guidance_scale=7.5, guidance_rescale=1.5)
    with pytest.raises(ValueError, match="guidance_rescale"):
        Sampler(None, "euler", 4, guidance_scale=7.5, guidance_rescale=-0.1)
    s = Sampler(None, "euler", 4, guidance_scale=7.5, guidance_rescale=0.7, prediction_type="v_prediction")
    assert s.rows_per_image == 2 and s.guidance_rescale == 0.7 and s.schedule.prediction_type == "v_prediction"
    s = Sampler(None, "ddim", 4, guidance_scale=7.5, image_guidance_scale=1.5, guidance_rescale=0.5)
    assert s.rows_per_image == 3
    assert Sampler(None, "euler", 4, guidance_scale=7.5).guidance_rescale == 0.0
