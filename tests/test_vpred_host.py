"""v-prediction and zero terminal SNR on the host (no GPU): the v-prediction tables are the epsilon tables composed with
eps = sqrt(1 - ac) x_vp + sqrt(ac) v; the solver keeps its order of convergence with the exact v oracle; a zero-SNR
schedule is finite, starts from pure noise and ends where the exact flow ends; the refused combinations; and the epsilon
tables are, bit for bit, those of the commit before the keywords existed (tests/golden/schedule_sha256.json)."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import multistep_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = ([(k, n, None, False) for k in ("euler_ancestral", "euler", "lcm") for n in (1, 4, 20)]
           + [("euler", 4, "trailing", False)]
           + [(k, n, sp, False) for k in ("ddim", "dpmpp_2m") for n in (1, 4, 20) for sp in ("leading", "trailing")]
           + [("dpmpp_2m", n, None, True) for n in (2, 6, 20)])


def _vp_pair(s, i):
    """(sqrt(ac), sqrt(1 - ac), scale of the state into VP space) at step i of an epsilon schedule."""
    from mixdq_amd.sampler import alphas_cumprod
    if s.sigmas is not None:
        alpha = 1.0 / np.sqrt(s.sigmas[i] ** 2 + 1.0)
        return alpha, s.sigmas[i] * alpha, (alpha if s.kind in ("euler", "euler_ancestral") else 1.0)
    ac = alphas_cumprod()[s.timesteps[i]]
    return np.sqrt(ac), np.sqrt(1.0 - ac), 1.0


# ---- the tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_v_rows_are_epsilon_rows_composed_with_the_conversion(cfg):
    """Float64, before the FP32 rounding: the v row applied to (x, v) equals the epsilon row applied to (x, eps(x, v))
    within 1e-12 of the larger of the two terms -- the update of the order-1 kinds, x0 of 'dpmpp_2m'."""
    from mixdq_amd.sampler import Schedule
    kind, n, spacing, karras = cfg
    se, sv = Schedule(kind, n, spacing, karras), Schedule(kind, n, spacing, karras, prediction_type="v_prediction")
    assert se.coef64.dtype == np.float64 and np.array_equal(sv.coef, sv.coef64.astype(np.float32))
    assert np.array_equal(se.t_table, sv.t_table) and np.array_equal(se.blend, sv.blend)
    assert (se.init_scale, se.input_scale0, se.uses_noise) == (sv.init_scale, sv.input_scale0, sv.uses_noise)
    assert np.array_equal(se.coef64[:, 2:], sv.coef64[:, 2:])            # c, s_next; A, B1, B2, D2, s_next, 0
    rng = np.random.default_rng(n)
    x, v = rng.standard_normal(64) * 3.0, rng.standard_normal(64)
    for i in range(n):
        sa, s1a, to_vp = _vp_pair(se, i)
        eps = s1a * (x * to_vp) + sa * v
        want = se.coef64[i, 0] * x + se.coef64[i, 1] * eps
        got = sv.coef64[i, 0] * x + sv.coef64[i, 1] * v
        scale = max(np.abs(se.coef64[i, 0] * x).max(), np.abs(se.coef64[i, 1] * eps).max())
        assert np.abs(got - want).max() <= 1e-12 * scale, (cfg, i)
    assert not np.array_equal(se.coef, sv.coef)


def test_epsilon_tables_hash_as_before():
    from mixdq_amd.sampler import Schedule
    with open(os.path.join(ROOT, "tests", "golden", "schedule_sha256.json")) as f:
        golden = json.load(f)
    assert len(golden) == len(CONFIGS)
    for kind, n, spacing, karras in CONFIGS:
        for s in (Schedule(kind, n, spacing, karras), Schedule(kind, n, spacing, karras, "epsilon", False)):
            h = hashlib.sha256()
            for a in (s.coef, s.t_table, s.blend):
                h.update(a.tobytes())
            assert h.hexdigest() == golden[f"{kind}/{n}/{spacing}/{int(karras)}"], (kind, n, spacing, karras)


# ---- the Gaussian model with the exact v oracle ------------------------------------------------------------------------
def _v_model(s):
    """Data ~ N(0, s^2): v = alpha * eps - sigma_hat * x0 with the exact eps of multistep_ref.gaussian_model."""
    eps = M.gaussian_model(s)

    def v(x, sigma):
        alpha = 1.0 / np.sqrt(sigma ** 2 + 1.0)
        hat = sigma * alpha
        e = eps(x, sigma)
        return alpha * e - hat * (x - hat * e) / alpha
    return v


@pytest.mark.parametrize("s", [0.5, 1.0, 2.0])
def test_second_order_convergence_with_the_v_oracle(s):
    """tests/test_multistep_host.py's experiment with the table's (u, v) = (alpha, -sigma_hat) and the exact v: the same
    bracket -- halving the step divides the second-order error by >= 3.5 and the first-order one by <= 2.2.  Measured
    ratios (n = 32 -> 64 -> 128): s 0.5: second order 4.03, 4.06, first order 1.99, 2.00; s 1.0: 4.02, 4.04 and 2.00,
    2.00; s 2.0: 3.95, 4.01 and 2.00, 2.00 -- the behaviour of the epsilon table on the same ladder."""
    from mixdq_amd.sampler import multistep_table
    x_T = np.linspace(-3.0, 3.0, 13)
    err = {True: [], False: []}
    for n in (32, 64, 128):
        sig = np.concatenate([np.geomspace(10.0, 1e-3, n), [0.0]])
        tab = multistep_table(sig)
        alpha = 1.0 / np.sqrt(sig[:-1] ** 2 + 1.0)
        tab[:, 0], tab[:, 1] = alpha, -sig[:-1] * alpha
        exact = M.gaussian_exact(x_T, sig[0], s)
        for second in (True, False):
            err[second].append(float(np.abs(M.table_2m(_v_model(s), x_T, tab, sig, second_order=second) - exact).max()))
    r2 = [err[True][i] / err[True][i + 1] for i in range(2)]
    r1 = [err[False][i] / err[False][i + 1] for i in range(2)]
    print(f"s {s}: second-order errors {err[True]} ratios {r2}; first-order errors {err[False]} ratios {r1}")
    assert min(r2) >= 3.5, r2
    assert max(r1) <= 2.2, r1
    assert err[True][0] < err[False][0]


# ---- zero terminal SNR ---------------------------------------------------------------------------------------------
def _run(sched, s, x, first_order=1):
    """A float64 run of `sched`'s table from state x with the exact v of data ~ N(0, s^2), written in (alpha, sigma_hat)
    so that alpha == 0 is an ordinary point: v = alpha hat x (1 - s^2) / (alpha^2 s^2 + hat^2).  -> (end state, the
    exact flow's end state).  first_order: how many leading rows of a 'dpmpp_2m' table are taken first-order."""
    from mixdq_amd.sampler import alphas_cumprod
    ac = alphas_cumprod(sched.zero_snr)
    pairs = [(np.sqrt(ac[t]), np.sqrt(1.0 - ac[t])) for t in sched.timesteps]
    tab, hist = sched.coef64, None
    spread = lambda a, h: np.sqrt(a * a * s * s + h * h)          # the std of the marginal at (alpha, hat)
    start = spread(*pairs[0])
    for i, (a, h) in enumerate(pairs):
        v = a * h * x * (1.0 - s * s) / (a * a * s * s + h * h)
        if sched.order == 2:
            p = tab[i, 0] * x + tab[i, 1] * v
            x = tab[i, 2] * x + (tab[i, 4] * p + tab[i, 5] * hist if i >= first_order and tab[i, 5] != 0.0 else tab[i, 3] * p)
            hist = p
        else:
            x = tab[i, 0] * x + tab[i, 1] * v
    end = (1.0, 0.0) if sched.order == 2 else (np.sqrt(ac[0]), np.sqrt(1.0 - ac[0]))      # ddim: set_alpha_to_one False
    return x, None if start == 0 else spread(*end) / start


def test_zero_snr_betas():
    from mixdq_amd.sampler import alphas_cumprod
    ac, plain = alphas_cumprod(True), alphas_cumprod()
    assert ac[-1] == 0.0 and ac[0] == pytest.approx(plain[0], rel=1e-12) and (np.diff(ac) < 0).all() and ac[-2] > 0
    assert plain[-1] > 0 and np.array_equal(plain, alphas_cumprod(False))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 20, 50])
@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m"])
def test_zero_snr_tables_are_finite_and_start_from_pure_noise(kind, n):
    from mixdq_amd.sampler import Schedule
    s = Schedule(kind, n, "trailing", prediction_type="v_prediction", zero_snr=True)
    assert s.timesteps[0] == 999 and s.sigmas is None
    for a in (s.coef, s.coef64, s.t_table, s.blend):
        assert np.isfinite(a).all()
    assert s.start(0) == (0.0, 1.0, 1.0) and s.init_scale == 1.0 and s.input_scale0 == 1.0
    assert s.blend[-1].tolist() == [1.0, 0.0]
    if kind == "dpmpp_2m":
        assert s.coef64[0, 0] == 0.0 and s.coef64[0, 1] == -1.0 and s.coef64[0, 5] == 0.0      # x0 = -v: first order
        if n > 2:
            assert s.coef64[1, 5] == 0.0 and s.coef64[1, 4] == s.coef64[1, 3]                   # r = infinity
        if n > 3:
            assert (s.coef64[2:-1, 5] < 0).all()
    else:
        assert s.coef64[0, 0] == pytest.approx(np.sqrt(1.0 - (s.coef64[0, 1]) ** 2))           # (sq, -sp): a rotation


@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("s", [0.5, 2.0])
def test_zero_snr_run_ends_where_the_flow_ends(kind, s):
    """From pure noise x_T (zero SNR: the data's share is exactly 0) the exact flow of data ~ N(0, s^2) ends at x_T times
    the end marginal's spread.  The bound is the error of the SAME solver on the schedule without zero SNR, from the same
    x_T at its own first step, against its own exact end: the rescaled betas move every step a little, so the two errors
    agree in size, not in digits -- the zero-SNR error may be at most twice the other, and both shrink with n.
    Like is compared with like: a zero-SNR 'dpmpp_2m' run takes its first TWO steps first-order (r is infinite at the
    second), so the run without zero SNR is given the same orders.  (Against a run with one first-order step the
    zero-SNR error is 2.04 times the other at s = 2, n = 20: the price of that step, not of the schedule.)"""
    from mixdq_amd.sampler import Schedule, multistep_table_vp
    x_T = np.linspace(-3.0, 3.0, 13)
    errs = {}
    for n in (20, 40):
        for zero in (False, True):
            sched = Schedule(kind, n, "trailing", prediction_type="v_prediction", zero_snr=zero)
            got, ratio = _run(sched, s, x_T, first_order=2)
            errs[n, zero] = float(np.abs(got - x_T * ratio).max())
        print(f"{kind} s {s} n {n}: plain {errs[n, False]:.3e}, zero SNR {errs[n, True]:.3e}")
        assert errs[n, True] <= 2.0 * errs[n, False]
    assert errs[40, True] < errs[20, True]
    # the (alpha, sigma_hat) form of the table is multistep_table's where both exist
    plain = Schedule("dpmpp_2m", 20, "trailing", prediction_type="v_prediction")
    alpha = 1.0 / np.sqrt(plain.sigmas ** 2 + 1.0)
    assert np.allclose(multistep_table_vp(alpha, plain.sigmas * alpha), plain.coef64, rtol=1e-10, atol=1e-13)


def test_refused_combinations():
    from mixdq_amd.sampler import Sampler, Schedule
    ok = dict(prediction_type="v_prediction", zero_snr=True)
    Schedule("ddim", 4, "trailing", **ok), Schedule("dpmpp_2m", 4, "trailing", **ok)
    with pytest.raises(ValueError, match="v_prediction"):
        Schedule("ddim", 4, "trailing", zero_snr=True)
    with pytest.raises(ValueError, match="VP space"):
        Schedule("euler", 4, "trailing", **ok)
    with pytest.raises(ValueError, match="VP space"):
        Schedule("euler_ancestral", 4, "trailing", **ok)
    with pytest.raises(ValueError, match="VP space"):
        Schedule("lcm", 4, **ok)
    with pytest.raises(ValueError, match="VP space"):
        Schedule("dpmpp_2m", 4, None, True, **ok)
    for spacing in (None, "leading"):
        with pytest.raises(ValueError, match="trailing"):
            Schedule("ddim", 4, spacing, **ok)
    with pytest.raises(ValueError, match="prediction_type"):
        Schedule("ddim", 4, prediction_type="sample")
    sm = Sampler(None, "ddim", 4, guidance_scale=7.5, spacing="trailing", guidance_rescale=0.7, **ok)
    assert sm.schedule.zero_snr and sm.schedule.prediction_type == "v_prediction" and sm.rows_per_image == 2
    with pytest.raises(ValueError, match="trailing"):
        Sampler(None, "ddim", 4, guidance_scale=7.5, **ok)
