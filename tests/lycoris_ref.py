"""numpy restatement (float64) of mixdq_lycoris_requant's arithmetic, include/mixdq_math.h mixdq_lycoris_*: the only
reference of the LoHa / DoRA tests.  Arrays are in LOGICAL row order; a layer is a dict with W, B, A, B2, A2 (f16; ranks
[0, r_lin) linear, then one range per entry of `ends`), svec, m (FP32 [N] or None) and the quantizer's fields."""
import numpy as np

from tests.lora_ref import F16, F32, F64, pack_w4

U = 2.0 ** -24


def merged(L):
    """(w' in float64, the absolute error bound of the kernel's FP32 w').  Bs = f16(svec * Bcat), rounded ONCE.  Bound:
    a sum of r products accumulated in FP32 errs by at most r u times the sum of their magnitudes; a Hadamard term is a
    product of two such sums and one fma, (2 r + 1) u M1 M2; one more u for what the accumulator already holds."""
    bs = (L["svec"].astype(F64)[None, :] * L["B"].astype(F64)).astype(F16).astype(F64)
    bs[:, L["svec"] == 0] = 0
    A, r = L["A"].astype(F64), L["r_lin"]
    wp = L["W"].astype(F64) + bs[:, :r] @ A[:r]
    err = (r + 2) * U * (np.abs(L["W"].astype(F64)) + np.abs(bs[:, :r]) @ np.abs(A[:r]))
    for a, b in zip([r] + list(L["ends"][:-1]), L["ends"]):
        b2, a2 = L["B2"][:, a:b].astype(F64), L["A2"][a:b].astype(F64)
        wp = wp + (bs[:, a:b] @ A[a:b]) * (b2 @ a2)
        err = (err + (2 * (b - a) + 1) * U * (np.abs(bs[:, a:b]) @ np.abs(A[a:b])) * (np.abs(b2) @ np.abs(a2))) * (1 + U)
    return wp, err


def requant(L, act_scale, act_zp, delta=None):
    """Everything the launch writes for one layer, plus the float64 quotient `quot`, `tau` (the half-width of the band
    around it the kernel's own quotient lies in) and `g_rel` (the relative error bound of g = m / sqrt(sum w'^2): the
    sum's own (16 ceil(Kf / 256) + 5) u and the w' errors, halved by the root, two roundings).  g = 1 without a magnitude
    and where the sum is 0.  `delta`: these per-row scales instead of the rule's."""
    wp, err = merged(L)
    g, g_rel = np.ones(len(wp)), np.zeros(len(wp))
    if L["m"] is not None:
        ss = (wp * wp).sum(axis=1)
        safe = np.where(ss > 0, ss, 1.0)
        rel = 0.5 * ((16 * -(-wp.shape[1] // 256) + 5) * U + 2 * (np.abs(wp) * err).sum(axis=1) / safe) + 2 * U
        g, g_rel = np.where(ss > 0, L["m"].astype(F64) / np.sqrt(safe), 1.0), np.where(ss > 0, rel, 0.0)
    ws = g[:, None] * wp
    w32 = ws.astype(F32)                                       # mul_rn(g, w'): exact inputs make both factors FP32 values
    tol = np.abs(g)[:, None] * err + np.abs(ws) * (g_rel + 2 * U)[:, None]
    if L["mode"] == "f16":
        return dict(out=w32.astype(F16), ws=ws, tol=tol)
    qmax = 2 ** (L["bits"] - 1) - 1
    if delta is None:
        delta = L["old_scales"].astype(F32)
        if L["rule"] == "absmax":
            mx = (np.abs(g) * np.abs(wp).max(axis=1)).astype(F32)
            delta = np.where(mx > 0, mx / F32(qmax), delta).astype(F32)
    # an 8-bit quantizer multiplies by the FP32 reciprocal (torch.quantize_per_channel), a narrower one divides (Path A)
    q32 = w32 * (F32(1) / delta)[:, None] if L["bits"] == 8 else w32 / delta[:, None]
    quot = ws * (F32(1) / delta).astype(F64)[:, None] if L["bits"] == 8 else ws / delta.astype(F64)[:, None]
    q = np.clip(np.rint(q32), -qmax - 1, qmax).astype(np.int8)
    taps = q.reshape(q.shape[0], -1, L["tap_len"]).astype(np.int64).sum(axis=2)
    return dict(out=q if L["mode"] == "int8" else pack_w4(q), q=q, quot=quot, tau=tol / delta.astype(F64)[:, None],
                g_rel=g_rel, weight_scales=delta, wsum=taps.astype(F32), bias0=taps.sum(axis=1).astype(F32) * F32(act_zp),
                scale=delta * F32(act_scale))
