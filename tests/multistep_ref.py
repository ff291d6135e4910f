"""The multistep sampler step (mixdq_sampler_step_2m; arithmetic: include/mixdq_math.h) restated in numpy float32 --
every operation one IEEE binary32 round-to-nearest ufunc call, in the specification's order -- and DPM-Solver++ 2M
itself in float64, written from its log / exp form and NOT through the coefficient table, with the analytic model
the order-of-convergence tests integrate."""
import numpy as np

f32 = np.float32


# ---- the FP32 restatement ------------------------------------------------------------------------------------------
def x0(x, e, u, v):
    """mixdq_sampler_x0: (u*x) + (v*e)."""
    with np.errstate(invalid="ignore", over="ignore"):
        ux = f32(u) * np.asarray(x, f32)
        ve = f32(v) * np.asarray(e, f32)
        return ux + ve


def update_2m(x, p, h, A, B, D):
    """mixdq_sampler_update_2m: ((A*x) + (B*x0)) + (D*h)."""
    with np.errstate(invalid="ignore", over="ignore"):
        ax = f32(A) * np.asarray(x, f32)
        bp = f32(B) * np.asarray(p, f32)
        dh = f32(D) * np.asarray(h, f32)
        s = ax + bp
        return s + dh


def update(x, p, A, B):
    """mixdq_sampler_update on the data prediction: (A*x) + (B*x0)."""
    with np.errstate(invalid="ignore", over="ignore"):
        ax = f32(A) * np.asarray(x, f32)
        bp = f32(B) * np.asarray(p, f32)
        return ax + bp


def guided(eps_u, eps_c, g):
    e = eps_u.astype(f32)
    if eps_c is not None:
        d = eps_c.astype(f32) - e
        gd = f32(g) * d
        e = e + gd
    return e


def step(x, hist, eps_u, eps_c, row, g, second):
    """One launch without the blend.  x, hist fp32 (hist is not looked at unless `second`), eps_u / eps_c fp16 (eps_c
    None: rows_per_image == 1), row = (u, v, A, B1, B2, D2, s_next, 0) fp32, second: step > first and D2 != 0, decided
    by the caller as the kernel decides it -> (next state fp32, new hist = x0 fp32)."""
    u, v, A, B1, B2, D2 = (f32(c) for c in row[:6])
    x = np.asarray(x, f32)
    p = x0(x, guided(eps_u, eps_c, g), u, v)
    return (update_2m(x, p, hist, A, B2, D2) if second else update(x, p, A, B1)), p


def is_second(row, i, first):
    return bool(i > first and f32(row[5]) != 0)


def scaled_input(x, s_next):
    with np.errstate(over="ignore"):
        return (np.asarray(x, f32) * f32(s_next)).astype(np.float16)


# ---- DPM-Solver++ 2M in float64, from its own formulas -------------------------------------------------------------
def direct_2m(model, x, sigmas, start=0, second_order=True):
    """x_T -> x_0 over the falling ladder `sigmas` (n + 1 values, the last 0) from step `start`: with alpha = 1 /
    sqrt(sigma^2 + 1), sigma_hat = sigma * alpha, lambda = log(alpha / sigma_hat), x0 = (x - sigma_hat * eps) / alpha,
        h = lambda' - lambda,  r = (lambda - lambda_prev) / h,  D0 = m0,  D1 = (m0 - m1) / r
        x' = (sigma_hat' / sigma_hat) x - alpha' (e^-h - 1) D0 - 1/2 alpha' (e^-h - 1) D1
    first-order (no D1 term) on the first executed step and on the last, where sigma' = 0 and x' = x0.
    model(x, sigma) is the epsilon prediction at the VP state x."""
    sig = np.asarray(sigmas, dtype=np.float64)
    n = len(sig) - 1
    x = np.asarray(x, dtype=np.float64)
    m1 = None
    for i in range(start, n):
        a, a_n = 1.0 / np.sqrt(sig[i] ** 2 + 1.0), 1.0 / np.sqrt(sig[i + 1] ** 2 + 1.0)
        sh, sh_n = sig[i] * a, sig[i + 1] * a_n
        m0 = (x - sh * model(x, sig[i])) / a
        if i == n - 1:
            x = m0
        else:
            lam, lam_n = np.log(a / sh), np.log(a_n / sh_n)
            h = lam_n - lam
            nxt = (sh_n / sh) * x - a_n * (np.exp(-h) - 1.0) * m0
            if second_order and i > start:
                lam_p = np.log(1.0 / sig[i - 1])             # alpha / sigma_hat = 1 / sigma
                r = (lam - lam_p) / h
                nxt = nxt - 0.5 * a_n * (np.exp(-h) - 1.0) * ((m0 - m1) / r)
            x = nxt
        m1 = m0
    return x


def table_2m(model, x, tab, sigmas, start=0, second_order=True):
    """The same run through a float64 coefficient table, as the kernel walks it."""
    x = np.asarray(x, dtype=np.float64)
    hist = None
    for i in range(start, len(tab)):
        u, v, A, B1, B2, D2 = tab[i, :6]
        p = u * x + v * model(x, sigmas[i])
        if second_order and i > start and D2 != 0.0:
            x = A * x + B2 * p + D2 * hist
        else:
            x = A * x + B1 * p
        hist = p
    return x


def gaussian_model(s):
    """Data ~ N(0, s^2): in VP space the exact epsilon is x * sqrt(sigma^2 + 1) * sigma / (s^2 + sigma^2)."""
    return lambda x, sigma: x * np.sqrt(sigma ** 2 + 1.0) * sigma / (s ** 2 + sigma ** 2)


def gaussian_exact(x_T, sigma0, s):
    """Where the probability-flow ODE of that model takes x_T from sigma0 to 0."""
    return x_T * np.sqrt(sigma0 ** 2 + 1.0) * s / np.sqrt(s ** 2 + sigma0 ** 2)
