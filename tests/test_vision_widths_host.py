"""The inputs of tests/test_vision_widths_gpu.py and, without a GPU, the proof that they can tell a right patch-embed
launch from a wrong one: the widths cover every clip_patch_embed_kernel<MAXT> with spare tiles and without; a LayerNorm
whose row sums drop a 16-column tile, count one twice or take in the spare tiles' accumulators leaves the test's
tolerance at most of a row; and the float64 restatement of the pixel fma is exact for the float pixels drawn."""
from fractions import Fraction

import numpy as np
import pytest

from tests import vision_ref

U = 2.0 ** -24                                # unit roundoff of FP32
MAXTS = (4, 12, 16, 20, 32)                   # csrc/clip_vision.hip: the instantiations, picked as the smallest >= N / 64
WIDTHS = {4: (192, 256), 12: (320, 576, 768), 16: (832, 1024), 20: (1088, 1280), 32: (1344, 1728, 2048)}
ALL_N = tuple(N for maxt in MAXTS for N in WIDTHS[maxt])
LN_CASES = tuple((5, N) for N in ALL_N) + ((1, 1024), (1, 2048))
EPS = 1e-5


def maxt_of(N):
    return min(m for m in MAXTS if m >= N // 64)


def exact_inputs(g, N, B):
    """tests/test_vision_gpu.py test_exact_inputs_bit_for_bit's recipe: |e| <= 3 * 588 + 8 < 2048 at any N."""
    rng = np.random.default_rng(100 * g + N + B)
    img = rng.integers(0, 4, (B, 3, 14 * g, 14 * g)).astype(np.uint8)
    w = rng.integers(-1, 2, (N, 3, 14, 14)).astype(np.float16)
    cls, pos = (rng.integers(-8, 9, s).astype(np.float16) for s in ((N,), (g * g + 1, N)))
    return img, w, cls, pos


def planted(N):
    """Per column: differs from one 16-column tile to the next and from one wave's quarter of the row to the next."""
    n = np.arange(N)
    return 1 + ((n // 16) % 7) + 3 * (n // (N // 4))


def ln_inputs(g, N, B=2):
    """-> dict(img uint8, norm, w, cls, pos, gamma, beta).  Pixels in [0, 1] against weights of mean 0.01: the product is
    about 3 in every column, so an accumulator that should not count shows in a row sum; `planted` rides on pos; the
    class row is 1.5 + 2.0 in every column: variance 0."""
    rng = np.random.default_rng(1000 * g + N)
    img = rng.integers(0, 256, (B, 3, 14 * g, 14 * g)).astype(np.uint8)
    w = (0.01 + 0.02 * rng.standard_normal((N, 3, 14, 14))).astype(np.float16)
    pos = rng.standard_normal((g * g + 1, N))
    pos[1:] += planted(N)
    pos[0] = 2.0
    gamma, beta = ((o + s * rng.standard_normal(N)).astype(np.float16) for o, s in ((1, 0.2), (0, 0.3)))
    return dict(img=img, norm=[(1.0 / 255.0, 0.0)] * 3, w=w, cls=np.full(N, 1.5, np.float16), pos=pos.astype(np.float16),
                gamma=gamma, beta=beta)


def ln_tolerance(e, gamma, beta, eps=EPS):
    """-> (y float64, tol): tests/test_vision_gpu.py test_layernorm_stage_on_a_known_input's bound, a function of N."""
    N = e.shape[-1]
    y, xhat, rstd = vision_ref.layernorm(e, gamma, beta, eps)
    amax = np.abs(e.astype(np.float64)).max(-1, keepdims=True)
    slack = np.abs(gamma.astype(np.float64)) * ((N + 2) * U * amax * rstd + (N + 8) * U * np.abs(xhat)) + U * np.abs(y)
    return y, np.spacing(np.abs(y).astype(np.float16)).astype(np.float64) + slack


def fma_pixels(dtype, seed=6, g=4, B=2):
    """Float pixels k / 8, 0 <= k <= 2040: FP16 values, the FP32 ones the same numbers."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2041, (B, 3, 14 * g, 14 * g)) / 8.0).astype(np.float16).astype(dtype)


def fma_norms():
    from mixdq_amd.vision import pixel_norm
    return {"clip": pixel_norm(), "pm1": [(2.0 / 255.0, -1.0)] * 3}


def one_tap_filter(N):
    """tests/test_vision_gpu.py test_normalisation_bit_for_bit's: column n is a single 1 at tap 37 n % 588."""
    w = np.zeros((N, 588), np.float16)
    w[np.arange(N), (37 * np.arange(N)) % 588] = 1
    return w.reshape(N, 3, 14, 14)


def wrong_layernorm(e, gamma, beta, weight, extra=0.0, eps=EPS):
    """float64 LayerNorm whose two row sums count column n weight[n] times (all 1: the right one) and whose first sum
    takes `extra` [.., 1] in besides; both still divide by N."""
    e = e.astype(np.float64)
    N = e.shape[-1]
    d = e - ((e * weight).sum(-1, keepdims=True) + extra) / N
    rstd = 1.0 / np.sqrt((d * d * weight).sum(-1, keepdims=True) / N + eps)
    return d * rstd * gamma.astype(np.float64) + beta.astype(np.float64)


def test_widths_run_every_instantiation_full_and_with_spare_tiles():
    assert len(set(ALL_N)) == len(ALL_N) == 12
    for maxt in MAXTS:
        nts = [N // 64 for N in WIDTHS[maxt]]
        assert all(N % 64 == 0 and maxt_of(N) == maxt for N in WIDTHS[maxt])
        assert max(nts) == maxt and min(nts) < maxt                                   # full, and with spare tiles
        if maxt > 4:                         # (N = 64, 128 run in tests/test_vision_gpu.py)
            assert min(nts) == max(m for m in MAXTS if m < maxt) + 1                  # the smallest N that selects it
    assert {N for g, N in LN_CASES if g == 5} == set(ALL_N)


@pytest.mark.parametrize("g,N", LN_CASES)
def test_wrong_row_sums_leave_the_tolerance(g, N):
    """The GPU test compares with float64 LayerNorm of e inside ln_tolerance.  Here e is the restatement's; every
    wrong LayerNorm must be OUTSIDE that tolerance at more than half of every row, the class row included."""
    a = ln_inputs(g, N)
    e, acc, _ = vision_ref.embed(a["img"], a["norm"], a["w"], a["cls"], a["pos"])
    y, tol = ln_tolerance(e, a["gamma"], a["beta"])
    assert np.ptp(e[:, 0].astype(np.float32)) == 0
    quarter, nt = N // 4, N // 64

    def share(bad):                          # per row: the share of elements outside the tolerance
        return (np.abs(bad - y) > tol).mean(-1)
    worst = 1.0
    for tile in range(N // 16):              # one tile of one wave left out
        wt = np.ones(N)
        wt[16 * tile:16 * tile + 16] = 0
        worst = min(worst, share(wrong_layernorm(e, a["gamma"], a["beta"], wt)).min())
    assert worst > 0.5, f"a dropped tile stays inside the tolerance at {1 - worst:.0%} of a row"
    for wave in range(4):                    # the last real tile of one wave counted twice
        wt = np.ones(N)
        wt[(wave + 1) * quarter - 16:(wave + 1) * quarter] = 2
        worst = min(worst, share(wrong_layernorm(e, a["gamma"], a["beta"], wt)).min())
    assert worst > 0.5, f"a tile counted twice stays inside the tolerance at {1 - worst:.0%} of a row"
    spare = maxt_of(N) - nt
    if spare:
        # What a sum loop over t < MAXT takes in: per wave, `spare` more copies of the last real tile's accumulators, the
        # product alone (pos is added to real tiles only).  The class block's spare accumulators are zeros: body rows.
        last = np.concatenate([acc[..., (wv + 1) * quarter - 16:(wv + 1) * quarter] for wv in range(4)], axis=-1)
        bad = wrong_layernorm(e[:, 1:], a["gamma"], a["beta"], np.ones(N), extra=spare * last.sum(-1, keepdims=True))
        worst = min(worst, (np.abs(bad - y[:, 1:]) > tol[:, 1:]).mean(-1).min())
        assert worst > 0.5, f"spare tiles in the mean stay inside the tolerance at {1 - worst:.0%} of a row"
    print(f"g {g} N {N}: the least share of a row outside the tolerance, over every wrong sum: {worst:.1%}")


def test_the_float64_pixel_fma_is_exact_for_the_drawn_values():
    """vision_ref.embed states f32(fma(u, a, b)) as float64 u * a + b rounded to FP32: one rounding only if the float64
    product and sum are exact.  Every value fma_pixels can draw, each channel of both norms, in rational arithmetic."""
    drawn = (np.arange(2041) / 8.0).astype(np.float16)
    assert np.array_equal(drawn.astype(np.float64), np.arange(2041) / 8.0)
    for dtype in (np.float16, np.float32):
        px = fma_pixels(dtype)
        assert px.dtype == dtype and np.isin(px.astype(np.float64), drawn.astype(np.float64)).all()
        assert np.array_equal(px.astype(np.float16).astype(dtype), px) and len(np.unique(px)) > 1500
    for norm in fma_norms().values():
        for a, b in np.asarray(norm, np.float32).astype(np.float64):
            got = drawn.astype(np.float64) * a + b
            assert all(Fraction(float(u)) * Fraction(float(a)) + Fraction(float(b)) == Fraction(float(s))
                       for u, s in zip(drawn, got))
