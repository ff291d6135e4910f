"""Guidance rescale (mixdq_sampler_step_rescaled; arithmetic: include/mixdq_math.h, mixdq_rescale_*) restated in numpy
float32: every operation below is one IEEE binary32 round-to-nearest ufunc call, and every sum runs in the
specification's order -- the lane's 8 elements in storage order, the 64 lanes of a wave as the balanced tree over
lane ^ 1, 2, .. 32, the four waves ((w0 + w1) + w2) + w3, the chunks of an image in chunk order by Chan's update.
The rest of a step is the existing restatements', which take the rescaled FP32 output in the place of a one-row FP16
one: tests/sampler_ref.py, multistep_ref.py, inpaint_ref.py (as tests/ip2p_ref.py uses them).

Accuracy of the rule itself (tests/test_rescale_host.py::test_specification_accuracy, measured there): s = sqrt(M2_t /
M2_e) against float64 std(ddof=1) on FP16-rounded N(mu, 1) data, mu in {0, 64, 1000}, n_image in {252, 2072, 16384,
65536}: at most 8.6e-8 relative over the twelve inputs (the bound asked is 1e-5; the fixed summation order changes
nothing material against a plain float32 model of the chunked rule, which stays below 3e-7); a float32 E[x^2] - mean^2
on the same data: up to 6.4e-8 at mu = 0, 2.6e-5 .. 2.9e-4 at mu = 64 and 1.8 .. 7.6 % at mu = 1000."""
import numpy as np

from tests import inpaint_ref as I
from tests import ip2p_ref as P
from tests import multistep_ref as M
from tests import sampler_ref as R

f32 = np.float32
CHUNK = 2048
_LANE = np.arange(64)


def ordered_sum(v):
    """S of the specification over the last axis (2048 values, absent ones already +0) -> one FP32 per leading index."""
    v = np.asarray(v, f32)
    a = v.reshape(v.shape[:-1] + (256, 8))
    with np.errstate(invalid="ignore", over="ignore"):
        s = a[..., 0] + a[..., 1]
        for j in range(2, 8):
            s = s + a[..., j]
        s = s.reshape(s.shape[:-1] + (4, 64))
        for k in (1, 2, 4, 8, 16, 32):
            s = s + s[..., _LANE ^ k]
        w = s[..., 0]
        return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def chunk_stats(v):
    """v: FP32 [n_image] -> (counts int64 [chunks], mean_c FP32 [chunks], M2_c FP32 [chunks])."""
    v = np.asarray(v, f32).reshape(-1)
    n = v.size
    chunks = (n + CHUNK - 1) // CHUNK
    pad = np.zeros(chunks * CHUNK, f32)
    pad[:n] = v
    pad = pad.reshape(chunks, CHUNK)
    present = (np.arange(chunks * CHUNK) < n).reshape(chunks, CHUNK)
    counts = present.sum(axis=1).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = ordered_sum(pad) / counts.astype(f32)
        d = pad - mean[:, None]
        sq = np.where(present, d * d, f32(0.0))
        return counts, mean, ordered_sum(sq)


def combine(counts, mean_c, m2_c):
    """mixdq_rescale_combine over the chunks in order, from (0, 0, 0) -> (mean, M2) FP32."""
    mean, m2, n = f32(0.0), f32(0.0), 0
    with np.errstate(invalid="ignore", over="ignore"):
        for k, mc, qc in zip(counts.tolist(), mean_c, m2_c):
            fn, fk, ft = f32(n), f32(k), f32(n + k)
            d = mc - mean
            w = fk / ft
            mean = mean + d * w
            q = (fn * fk) / ft
            dd = d * d
            m2 = m2 + (qc + dd * q)
            n += k
    return f32(mean), f32(m2)


def image_m2(v):
    return combine(*chunk_stats(v))[1]


def factor(m2_t, m2_e, phi, n_image):
    """mixdq_rescale_factor."""
    if m2_e == 0 or m2_t == 0 or n_image == 1:
        return f32(1.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.sqrt(f32(m2_t) / f32(m2_e))
        return f32(f32(1.0) + f32(phi) * (s - f32(1.0)))


def std_ratio(t, e):
    """s = sqrt(M2_t / M2_e) of one image, as FP32."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(image_m2(t) / image_m2(e))


def rescaled(rows, g, gi, phi, n_image):
    """rows: the FP16 row blocks, each [n] in storage order (2: (eps_u, eps_c); 3: (e_t, e_i, e_u)) -> (e' FP32 [n],
    r FP32 [images])."""
    if len(rows) == 3:
        t, e = np.asarray(rows[0]).astype(f32), P.guided_eps3(rows[0], rows[1], rows[2], g, gi)
    else:
        t, e = np.asarray(rows[1]).astype(f32), M.guided(np.asarray(rows[0]), np.asarray(rows[1]), g)
    t, e = t.reshape(-1, n_image), e.reshape(-1, n_image)
    r = np.array([factor(image_m2(tb), image_m2(eb), phi, n_image) for tb, eb in zip(t, e)], dtype=f32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (e * r[:, None]).reshape(-1), r


def step(x, rows, row, g, gi, phi, n_image, *, noise=None, hist=None, second=False, blend=None):
    """One mixdq_sampler_step_rescaled launch group; the arguments of ip2p_ref.step3 with the row blocks as a sequence.
    -> (state FP32, next input FP16, new hist or None)."""
    e, _ = rescaled(rows, g, gi, phi, n_image)
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
