"""Exact-result inputs for the FP16 attention core, the fused to_q + cross-attention launch, the FP16 layer kernels
and the norm producers (tests/test_attention_exact_gpu.py, tests/test_qlinear_attention_exact_gpu.py,
tests/test_f16_exact_gpu.py, tests/test_norm_exact_gpu.py run them on the GPU; tests/test_exact_inputs_host.py checks
them on the CPU).

The technique: inputs for which the mathematically exact result is also the only result a correct kernel can
produce, so that the comparison is equality of bits and needs no tolerance.  Every builder returns the inputs and the
expected output, and checks its own precondition in float64 (AssertionError if it does not hold).

Attention
  selection()        one-hot softmax.  Keys are sign codes k_j = a s_j, s_j in {-1, +1}^D, query i is a copy of key
                     j(i).  Precondition: in log2 units the hot scaled score exceeds every other key's by >= 26 -- every
                     other P is below 2^-25 and rounds to exactly 0 in FP16 -- and is <= 1000, so that the hot P is
                     1 to FP16 rounding.  The keys of EARLIER tiles still reach the FP32 accumulator through the
                     running-maximum rescale (factor <= 2^-26), as they reach the exact result; a further precondition
                     bounds that remainder, sum_j 2^-gap_j * max|v|, by 1/16 ulp of every expected FP16 value.  For
                     that, one (batch, head) holds values of one magnitude class: "unit" (1/32 .. 2), "huge"
                     (8192 .. 65504) or "subnormal" (nonzero multiples of 2^-24 below 2^-14).
                     Expected: out[i] == v[j(i)], bit for bit.
  every_key_once()   q = 0: every score 0, every P exactly 1.  One probe key per channel holds 2048, every other value
                     is 0: out = 2048 / tkv (a dropped key gives 0, a key counted twice -- or an unmasked re-read of the
                     last key -- twice the value).
  small_integers()   q = 0, v small integers, tkv a power of two, tkv * max|v| < 2^24: out = fp16(sum / tkv) exactly.
  rescale()          score staircases, a late dominant key, equal large scores, |v| near the FP16 maximum: float64
                     softmax as the expected output (tolerance-held; they drive the running-maximum rescale).
to_q + cross-attention (mixdq_qlinear_w8a8_attn: Q comes out of the INT8 GEMM, head width 64, at most 128 keys)
  toq_operands()     int8 a [B, T, K], int8 w [N, K] in [-2, 1] (the same integers pack to W8, W4 and W2), scale 1,
                     bias0 0, whose GEMM result IS the fp16 q of one of the builders above (asserted in int64):
                     a one-hot row of `a` per (image, head) picks the sign code of the hot key -- or, for rescale(),
                     the sign vector u -- out of w; for the q = 0 builders dense non-zero rows of `a` meet weight
                     columns in cancelling pairs.
FP16 layers
  linear() / conv2d() / gemm()   integer-valued activations in [-4, 4], weights in [-2, 2], bias a multiple of 1/8 in
                     [-4, 4]: |acc| < 2^20, so the FP32 accumulator and accumulator + bias are exact in any summation
                     order, and the result is fp16(acc + bias) [then fp16(f32(.) + f32(residual))] and nothing else.

Norm producers (csrc/fused_norm.hip; the builders are at the end of this file)
  gn_base() / gn_heavy()   integer data, one heavy element moved through the geometry's edges: the expected bits follow
                     from the kernel's order-free finalize tail (gn_expected).
  ln_heavy()         rows whose 16-column groups sum to zero (ln_expected_zero_mean), a heavy element moved through
                     the group, unit and lane-wrap boundaries; constant rows (ln_expected_constant).
  qedge_values()     values on the quantizers' ties and clamp ends.

Plain numpy; imports without a GPU and without the built library.
"""
import functools

import numpy as np

from tests import detdata as dd

LOG2E = 1.4426950408889634
WIDTHS = (64, 40, 80, 160)
AMPLITUDE = {40: 4.0, 64: 3.0, 80: 3.0, 160: 2.0}        # a of k_j = a s_j
# key counts: 1, whole and ragged tiles of 64, tkv % 64 in {1, 4, 5, 32, 33, 63} (96, 97, 196, 197), the ring's wrap
KEY_COUNTS = (1, 63, 64, 65, 77, 96, 97, 127, 128, 129, 130, 196, 197, 256, 300, 640, 1024, 4096, 4097)
TILE = 64
PROBE = 2048.0
MIN_GAP, MAX_HOT = 26.0, 1000.0
CLASSES = ("unit", "huge", "subnormal")


def query_count(tkv):
    """Ragged against the 64- and the 128-query workgroup; tq == tkv (the fused q|k|v layout) at three counts."""
    return tkv if tkv in (65, 130, 300) else 200


def boundary_keys(tkv):
    """The first and the last key, both sides of every 64-key tile boundary, and the last nine keys: both sides of
    the split between the two half-waves' groups of four (mask limit tkv - 64 t - 4 hh) and of the ragged end."""
    ks = {0, tkv - 1}
    for b in range(TILE, tkv, TILE):
        ks |= {b - 1, b}
    ks |= {tkv - 1 - i for i in range(9) if tkv - 1 - i >= 0}
    return sorted(ks)


def ulp16(x):
    """Spacing of the FP16 numbers at |x| (float64; 2^-24 for subnormals and zero; finite at the FP16 maximum)."""
    m, e = np.frexp(np.abs(np.asarray(x, np.float64)))          # |x| = m 2^e, m in [0.5, 1); (0, 0) for zero
    return np.exp2(np.where(m == 0, -14, np.maximum(e - 1, -14)).astype(np.float64) - 10)


def _shuffle(seed, n):
    return np.argsort(dd.u64(seed, n), kind="stable")


def hot_keys(tq, tkv, seed=0):
    """j(i): every key when tq >= tkv, else the boundary keys first and a spread of the others; the queries that
    carry them are shuffled (query position and key position are unrelated)."""
    if tq >= tkv:
        j = np.arange(tq) % tkv
    else:
        bl = boundary_keys(tkv)
        assert len(bl) <= tq, "more boundary keys than queries"
        j = np.array(bl + [(i * 2654435761 + 17) % tkv for i in range(tq - len(bl))])
    return j[_shuffle(seed + 7, tq)].astype(np.int64)


def _signs(seed, shape):
    n = int(np.prod(shape))
    return (((dd.u64(seed, n) >> np.uint64(40)) & np.uint64(1)).astype(np.float64) * 2 - 1).reshape(shape)


def class_values(cls, seed, shape):
    """FP16 values of one magnitude class, random signs, no zeros."""
    u, sg = dd.uniform01(seed, shape), _signs(seed + 1, shape)
    if cls == "unit":
        return (sg * (1 / 32 + u * (2 - 1 / 32))).astype(np.float16)
    if cls == "huge":
        return (sg * (8192 + u * (65504 - 8192))).astype(np.float16)
    # 1 .. 1023 units of 2^-24: subnormals.  No zeros: the remainder of the other keys, however small, decides the
    # SIGN of a zero result, in the exact arithmetic as in the kernel's
    return (sg * (1 + np.floor(u * 1023)) * 2.0 ** -24).astype(np.float16)


def _heads(x, heads):
    B, T, C = x.shape
    return x.reshape(B, T, heads, C // heads).transpose(0, 2, 1, 3)


def log2_scores(q, k, heads):
    """Scaled scores in log2 units, float64: [B, heads, Tq, Tkv]."""
    D = q.shape[-1] // heads
    return np.einsum("bhqd,bhkd->bhqk", _heads(q.astype(np.float64), heads), _heads(k.astype(np.float64), heads)
                     ) * (D ** -0.5 * LOG2E)


@functools.lru_cache(maxsize=4)
def selection(D, tkv, tq=None, B=2, heads=3, seed=0):
    tq = query_count(tkv) if tq is None else tq
    C = heads * D
    a = AMPLITUDE[D]
    k = (a * _signs(1000 + seed + D + 7 * tkv, (B, tkv, C))).astype(np.float16)
    v = np.empty((B, tkv, C), np.float16)
    hot = np.empty((B, heads, tq), np.int64)
    j = hot_keys(tq, tkv, seed)
    cls = {}
    for b in range(B):
        for h in range(heads):
            cls[b, h] = CLASSES[(b * heads + h) % 3]
            v[b, :, h * D:(h + 1) * D] = class_values(cls[b, h], 2000 + seed + 16 * (b * heads + h) + tkv, (tkv, D))
            hot[b, h] = j if (b * heads + h) % 2 == 0 else j[::-1]
    q = np.empty((B, tq, C), np.float16)
    expected = np.empty((B, tq, C), np.float16)
    for b in range(B):
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            q[b, :, sl] = k[b, hot[b, h], sl]
            expected[b, :, sl] = v[b, hot[b, h], sl]
    # ---- preconditions, float64 ----
    s = log2_scores(q, k, heads)
    stats = dict(min_gap=np.inf, max_hot=0.0, min_hot=np.inf, max_rest_ulps=0.0)
    for b in range(B):
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            sb = s[b, h]
            hs = sb[np.arange(tq), hot[b, h]]
            rel = sb - hs[:, None]
            rel[np.arange(tq), hot[b, h]] = -np.inf
            gap = -rel.max(axis=1) if tkv > 1 else np.full(tq, np.inf)
            assert (gap >= MIN_GAP).all(), f"selection D={D} tkv={tkv}: gap {gap.min():.1f} < {MIN_GAP}"
            assert (hs <= MAX_HOT).all() and (hs > 0).all(), f"selection D={D} tkv={tkv}: hot score {hs.max():.1f}"
            rest = np.exp2(rel).sum(axis=1) * np.abs(v[b, :, sl].astype(np.float64)).max()     # [tq]
            ulp = ulp16(expected[b, :, sl])                                                     # [tq, D]
            ratio = (rest[:, None] / ulp).max()
            assert ratio <= 1 / 16, f"selection D={D} tkv={tkv} ({cls[b, h]}): the other keys weigh {ratio:.3g} ulp"
            rows = v[b, :, sl].view(np.uint16)
            assert len(np.unique(rows, axis=0)) == tkv, "value rows are not distinct"
            stats["min_gap"] = min(stats["min_gap"], float(gap.min()))
            stats["max_hot"], stats["min_hot"] = max(stats["max_hot"], float(hs.max())), min(stats["min_hot"], float(hs.min()))
            stats["max_rest_ulps"] = max(stats["max_rest_ulps"], float(ratio))
    return dict(q=q, k=k, v=v, heads=heads, hot=hot, expected=expected, classes=cls, stats=stats)


def _zero_score_qk(D, tkv, tq, B, heads, seed):
    C = heads * D
    return np.zeros((B, tq, C), np.float16), dd.normal_f16(3000 + seed + D + tkv, (B, tkv, C), 1.2)


@functools.lru_cache(maxsize=4)
def every_key_once(D, tkv, tq=None, B=2, heads=3, seed=0):
    """expected is float64 2048 / tkv: the FP16 output must lie within one FP16 ulp of it (`ulp`), and equal it
    where tkv is a power of two (`exact`)."""
    tq = query_count(tkv) if tq is None else tq
    C = heads * D
    q, k = _zero_score_qk(D, tkv, tq, B, heads, seed)
    bl = boundary_keys(tkv)
    probes = np.array([bl[i % len(bl)] for i in range(B * C)]).reshape(B, C)       # J[b, h * D + d]
    v = np.zeros((B, tkv, C), np.float16)
    for b in range(B):
        v[b, probes[b], np.arange(C)] = PROBE
    expected = np.full((B, tq, C), PROBE / tkv, np.float64)
    e16 = expected.astype(np.float16)
    assert np.array_equal(v.astype(np.float64).sum(axis=1) / tkv, expected[:, 0])           # one probe per channel
    assert (log2_scores(q, k, heads) == 0).all()
    assert np.isfinite(e16).all() and (np.abs(e16) >= 2.0 ** -14).all()                        # a normal FP16 number
    exact = tkv & (tkv - 1) == 0
    assert not exact or np.array_equal(e16.astype(np.float64), expected)
    return dict(q=q, k=k, v=v, heads=heads, probes=probes, expected=expected, expected16=e16,
                ulp=ulp16(e16), exact=exact)


@functools.lru_cache(maxsize=4)
def small_integers(D, tkv, tq=None, B=2, heads=3, seed=0, vmax=64):
    assert tkv & (tkv - 1) == 0, "tkv must be a power of two"
    assert 0 < vmax <= 127, "values are drawn as int8"
    tq = query_count(tkv) if tq is None else tq
    C = heads * D
    q, k = _zero_score_qk(D, tkv, tq, B, heads, seed)
    vi = dd.int8(4000 + seed + D + tkv, (B, tkv, C), -vmax, vmax + 1).astype(np.int64)
    assert tkv * np.abs(vi).max() < 2 ** 24                 # every partial sum is an exact FP32 integer
    v = vi.astype(np.float16)
    assert np.array_equal(v.astype(np.int64), vi)
    mean = vi.sum(axis=1).astype(np.float64) / tkv          # exact: a power-of-two divisor
    assert np.array_equal(mean.astype(np.float32).astype(np.float64), mean)    # ... and an FP32 number: one rounding
    expected = np.broadcast_to(mean.astype(np.float16)[:, None, :], (B, tq, C)).copy()
    return dict(q=q, k=k, v=v, heads=heads, expected=expected, mean=mean)


def softmax_attention64(q, k, v, heads, scale=None):
    """Float64 softmax(q k^T scale) v per head, maximum subtracted: [B, Tq, C]."""
    B, tq, C = q.shape
    D = C // heads
    s = log2_scores(q, k, heads) / LOG2E * (1.0 if scale is None else scale * D ** 0.5)
    s -= s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    return np.einsum("bhqk,bhkd->bhqd", p, _heads(v.astype(np.float64), heads)).transpose(0, 2, 1, 3).reshape(B, tq, C)


RESCALE_KINDS = ("rise4", "rise40", "fall4", "fall40", "late_dominant", "equal_large", "equal_large_negative",
                 "huge_values")
RESCALE_KEY_COUNTS = (77, 300, 640)


@functools.lru_cache(maxsize=4)
def rescale(kind, D, tkv, tq=200, B=2, heads=2, seed=0, q_noise=0.25):
    """q = alpha u + noise, k_j = beta_j u + noise with u a sign vector: the scaled log2 score of key j is about
    alpha beta_j sqrt(D) log2(e), chosen per kind (a staircase over the 64-key tiles, a late dominant key, one
    large value for all).  Returns the float64 result as `expected` and the per-kind facts the host test checks.
    `q_noise`: the noise of q where the kind has any (0: q == alpha u exactly, the noise stays in k)."""
    assert kind in RESCALE_KINDS
    C = heads * D
    s0 = 5000 + seed + D + tkv + 97 * RESCALE_KINDS.index(kind)
    u = np.tile(_signs(s0, (1, 1, C)), (B, 1, 1))
    unit = D ** 0.5 * LOG2E                                  # log2 units of score per unit of alpha * beta
    tile = np.arange(tkv) // TILE
    nt = int(tile.max()) + 1
    noise = 0.25
    if kind in ("rise4", "rise40", "fall4", "fall40"):
        step = 40.0 if kind.endswith("40") else 4.0
        level = step * (tile if kind.startswith("rise") else (nt - 1 - tile))
    elif kind == "late_dominant":
        level = np.zeros(tkv)
        level[min(5, tkv - 1)] = 50.0                        # a large maximum in the first tile
        level[tkv - 2 if tkv > 1 else 0] = 100.0             # the dominant key, in the last
    elif kind == "equal_large":
        level, noise = np.full(tkv, 60.0), 0.0
    elif kind == "equal_large_negative":
        level, noise = np.full(tkv, -60.0), 0.0
    else:
        level, noise = np.zeros(tkv), 1.2
    if kind == "huge_values":
        q = dd.normal_f16(s0 + 1, (B, tq, C), 1.2)
        k = dd.normal_f16(s0 + 2, (B, tkv, C), 1.2)
        # one sign per channel: the exact result is itself near the FP16 maximum (no cancellation to ~0, which
        # would turn a relative bound into an absolute one of 2e-3 on sums of 6e4)
        mag = 3e4 + 3e4 * dd.uniform01(s0 + 3, (B, tkv, C))
        v = (mag * _signs(s0 + 4, (B, 1, C))).astype(np.float16)
    else:
        alpha = 2.0
        qn = q_noise if noise else 0.0
        q = (alpha * u + qn * dd.normal_f16(s0 + 1, (B, tq, C), 1.0).astype(np.float64)).astype(np.float16)
        beta = level / (alpha * unit)
        k = (beta[None, :, None] * u + noise * dd.normal_f16(s0 + 2, (B, tkv, C), 1.0).astype(np.float64)
             ).astype(np.float16)
        v = dd.normal_f16(s0 + 3, (B, tkv, C), 1.2)
    s = log2_scores(q, k, heads)
    assert np.isfinite(s).all() and np.abs(s).max() < 2000
    tmax = np.stack([s[..., tile == t].max(axis=-1) for t in range(nt)], axis=-1)      # [B, h, tq, nt]
    facts = dict(tile_max=tmax, max_abs_score=float(np.abs(s).max()))
    return dict(q=q, k=k, v=v, heads=heads, expected=softmax_attention64(q, k, v, heads), facts=facts, scores=s)


# ------------------------------------------------------------------------------------------ to_q + cross-attention
# The fused launch (csrc/igemm_kernel.h, ATT) computes Q itself: 64 x 128 x 128 tiles of an INT8 GEMM, three stages,
# the keys and values of a head pair staged by LDS-DMA ahead of the K-tiles.  The builders above prescribe a fp16 q;
# here the GEMM's operands are built so that it produces that q exactly.
#   K is cut into one block of 128 columns per (image, head): K = 128 B heads (1024: eight K-tiles at B = 2, heads = 4).
#   one-hot: row (b, i) of `a` holds the amplitude at column 128 (b heads + h) + col[b, h][i] for every head h and 0
#            elsewhere; w[n, block (b, h), j] is the sign the query must get at channel n (n inside head h) when it
#            addresses column j, and 0 for n outside that head.  Columns no row addresses hold non-zero filler from
#            {-2, -1, 1}: a mis-indexed K column gives a q that is no key.  acc = amplitude * sign, exactly.
#   zero:    a[b, i, 2 j] == a[b, i, 2 j + 1] (random, non-zero), w[n, 2 j + 1] == -w[n, 2 j] in {-1, 1}: every
#            accumulator is a sum of K / 2 cancelling pairs -- the GEMM multiplies, its result is 0.
QATT_KEY_COUNTS = (1, 4, 5, 63, 64, 65, 77, 96, 97, 127, 128)     # both sides of the half-wave mask split, of the tile
QATT_QUERY_COUNTS = (64, 192)                                     # whole 64-row tiles: one and three per image
QATT_B, QATT_HEADS, QATT_BLOCK = 2, 4, 128
QATT_RESCALE_KEY_COUNTS = (65, 77, 128)                           # two key tiles each
QATT_RESCALE_COLUMNS = 96                                         # addressed columns per block of the rescale() form


def _filler(seed, shape):
    n = int(np.prod(shape))
    return np.array([-2, -1, 1], np.int8)[((dd.u64(seed, n) >> np.uint64(35)) % np.uint64(3)).astype(np.int64)].reshape(shape)


def _one_hot_operands(amp, col, sign, B, T, heads, D, seed):
    """col [B, heads, T]: the addressed column of block (b, h) per query; sign [B, heads, D, ncol] in {-1, +1}: the
    weights of the addressed columns.  Returns a [B, T, K], w [heads D, K]."""
    ncol = sign.shape[-1]
    assert ncol <= QATT_BLOCK and col.max() < ncol and col.min() >= 0 and set(np.unique(sign)) <= {-1, 1}
    K = QATT_BLOCK * B * heads
    a = np.zeros((B, T, K), np.int8)
    w = np.zeros((heads * D, K), np.int8)
    for b in range(B):
        for h in range(heads):
            c0 = QATT_BLOCK * (b * heads + h)
            a[b, np.arange(T), c0 + col[b, h]] = amp
            w[h * D:(h + 1) * D, c0:c0 + ncol] = sign[b, h]
            if ncol < QATT_BLOCK:        # never addressed: non-zero at EVERY channel
                w[:, c0 + ncol:c0 + QATT_BLOCK] = _filler(seed + 31 * (b * heads + h), (heads * D, QATT_BLOCK - ncol))
    return a, w


def _zero_operands(B, T, N, K, seed):
    assert K % 2 == 0
    half = dd.int8(seed, (B, T, K // 2), 1, 128) * (2 * dd.int8(seed + 1, (B, T, K // 2), 0, 2) - 1)   # 1 .. 127, signed
    ws = (2 * dd.int8(seed + 2, (N, K // 2), 0, 2) - 1).astype(np.int8)
    a = np.repeat(half.astype(np.int8), 2, axis=2)
    w = np.stack([ws, -ws], axis=2).reshape(N, K)
    assert (a != 0).all() and (w != 0).all()
    return a, w


@functools.lru_cache(maxsize=4)
def toq_operands(family, tkv, tq=64, kind=None, B=QATT_B, heads=QATT_HEADS, seed=0):
    """The operands of to_q for one attention case at head width 64: dict(a int8 [B, tq, K], w int8 [N, K] with values
    in [-2, 1], scale, bias0 (float32 [N]: 1 and 0), q fp16 [B, tq, N] -- what the GEMM gives, bit for bit -- and
    `case`, the attention builder's own dict (k, v, expected, ...)).
    family: "selection" | "every_key_once" | "small_integers" | "rescale" (with `kind`, not "huge_values": its q is
    no sign vector)."""
    D = 64
    N = heads * D
    assert tq % 64 == 0 and 0 < tkv <= 2 * TILE
    if family == "selection":
        c = selection(D, tkv, tq, B, heads, seed)
        ksign = np.sign(_heads(c["k"].astype(np.float64), heads)).astype(np.int8)          # [B, heads, tkv, D]
        a, w = _one_hot_operands(int(AMPLITUDE[D]), c["hot"], ksign.transpose(0, 1, 3, 2), B, tq, heads, D, 6000 + seed + tkv)
    elif family == "rescale":
        assert kind in RESCALE_KINDS and kind != "huge_values"
        c = rescale(kind, D, tkv, tq, B, heads, seed, q_noise=0.0)
        u = np.sign(_heads(c["q"][:, :1].astype(np.float64), heads)).astype(np.int8)       # [B, heads, 1, D]
        sign = np.repeat(u.transpose(0, 1, 3, 2), QATT_RESCALE_COLUMNS, axis=3)
        col = np.broadcast_to((np.arange(tq) * 37 + 11) % QATT_RESCALE_COLUMNS, (B, heads, tq))
        a, w = _one_hot_operands(2, col, sign, B, tq, heads, D, 6100 + seed + tkv)
    else:
        c = {"every_key_once": every_key_once, "small_integers": small_integers}[family](D, tkv, tq, B, heads, seed)
        a, w = _zero_operands(B, tq, N, 512, 6200 + seed + tkv)
    assert w.min() >= -2 and w.max() <= 1, "the weights must pack to W2"
    assert (np.abs(a.astype(np.int64)).sum(axis=2) > 0).all(), "an all-zero activation row"
    acc = a.reshape(B * tq, -1).astype(np.int64) @ w.astype(np.int64).T                      # exact
    q = c["q"]
    assert np.array_equal(acc.reshape(B, tq, N).astype(np.float64), q.astype(np.float64)), "the GEMM does not give q"
    assert np.array_equal(acc.reshape(B, tq, N).astype(np.float16).view(np.uint16), q.view(np.uint16))
    return dict(a=a, w=w, scale=np.ones(N, np.float32), bias0=np.zeros(N, np.float32), q=q, case=c)


# ------------------------------------------------------------------------------------------ FP16 layers
def _ints16(seed, shape, lim):
    return dd.int8(seed, shape, -lim, lim + 1).astype(np.float16)


def _eighths(seed, shape):
    return (dd.int8(seed, shape, -32, 33).astype(np.float64) / 8).astype(np.float16)


def f16_epilogue(acc, bias, residual):
    """The F16 epilogue's rounding points (csrc/igemm_kernel.h): fp16(f32(acc) + f32(bias)), then -- the residual is
    added AFTER that rounding -- fp16(f32(.) + f32(residual)).  `acc`: exact integers, |acc| < 2^20 (asserted), so
    acc and acc + bias (a multiple of 1/8) are exact FP32 numbers and the first line is ONE rounding."""
    acc = np.asarray(acc)
    assert np.abs(acc).max(initial=0) < 2 ** 20, "accumulator not exact in FP32 with three fraction bits"
    r = acc.astype(np.float32)
    assert np.array_equal(r.astype(np.float64), acc.astype(np.float64))
    if bias is not None:
        exact = acc.astype(np.float64) + bias.astype(np.float64)
        r = r + bias.astype(np.float32)
        assert np.array_equal(r.astype(np.float64), exact)
    assert np.abs(r).max(initial=0) < 65504
    out = r.astype(np.float16)
    if residual is not None:
        out = (out.astype(np.float32) + residual.astype(np.float32)).astype(np.float16)
    return out


def _seed(*v):
    s = 12345
    for x in v:
        s = (s * 1000003 + int(x)) % (1 << 31)
    return s


@functools.lru_cache(maxsize=2)
def linear(M, K, N, bias=True, residual=False, seed=0):
    """x [M, K], w [N, K], bias [N] or None, residual [M, N] or None -> expected [M, N] fp16.  The accumulation runs
    in float64 (exact for these integers: |acc| <= 8 K < 2^53; tests/test_exact_inputs_host.py restates it in
    int64)."""
    s = _seed(M, K, N, seed)
    x, w = _ints16(s, (M, K), 4), _ints16(s + 1, (N, K), 2)
    b = _eighths(s + 2, (N,)) if bias else None
    res = _eighths(s + 3, (M, N)) if residual else None
    acc = x.astype(np.float64) @ w.astype(np.float64).T
    return dict(x=x, w=w, bias=b, residual=res, expected=f16_epilogue(acc, b, res))


def gemm(M, K, N, seed=0):
    """a [M, K] @ b [K, N] (mixdq_gemm_f16: no bias) -> expected [M, N] fp16."""
    s = _seed(M, K, N, seed, 77)
    a, b = _ints16(s, (M, K), 4), _ints16(s + 1, (K, N), 2)
    return dict(a=a, b=b, expected=f16_epilogue(a.astype(np.float64) @ b.astype(np.float64), None, None))


def conv_accumulate(x, w, stride, pad, dtype=np.float64):
    """sum_{c, r, s} x[n, c, p * stride + r - pad, q * stride + s - pad] * w[k, c, r, s]: [N, K, P, Q] in `dtype`."""
    N, Cin, H, W = x.shape
    K, _, R, S = w.shape
    P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    xp = np.zeros((N, Cin, H + 2 * pad, W + 2 * pad), dtype)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    wd = w.astype(dtype)
    acc = np.zeros((N, K, P, Q), dtype)
    for r in range(R):
        for s in range(S):
            win = xp[:, :, r:r + (P - 1) * stride + 1:stride, s:s + (Q - 1) * stride + 1:stride]   # [N, C, P, Q]
            acc += np.einsum("ncpq,kc->nkpq", win, wd[:, :, r, s], optimize=True)
    return acc


@functools.lru_cache(maxsize=2)
def conv2d(N, Cin, H, W, K, ks, stride, pad, bias=True, residual=None, seed=0):
    """x [N, C, H, W], w [K, C, R, S] (NCHW order), residual None | "full" ([N, K, P, Q]) | "per_image" ([N, K])
    -> expected [N, K, P, Q] fp16.  `ks`: the square kernel size, or (R, S) (a square size given as an int keeps the
    seed, and with it the data, it always had)."""
    if isinstance(ks, tuple):
        R, S = ks
        s = _seed(N, Cin, H, W, K, R, S, stride, pad, seed, 78)
    else:
        R = S = ks
        s = _seed(N, Cin, H, W, K, ks, stride, pad, seed)
    x, w = _ints16(s, (N, Cin, H, W), 4), _ints16(s + 1, (K, Cin, R, S), 2)
    b = _eighths(s + 2, (K,)) if bias else None
    acc = conv_accumulate(x, w, stride, pad)
    res = None
    if residual == "full":
        res = _eighths(s + 3, acc.shape)
    elif residual == "per_image":
        res = _eighths(s + 3, (N, K))
    rb = None if res is None else (res if residual == "full" else res[:, :, None, None])
    return dict(x=x, w=w, bias=b, residual=res,
                expected=f16_epilogue(acc, None if b is None else b[None, :, None, None], rb))


LIN = [  # M, K, N, bias: the shapes of tests/test_f16_gpu.py
    (1024, 5120, 1280, True), (203, 1232, 136, True), (331, 1280, 424, False), (77, 2048, 640, False),
    (1, 1280, 1280, True), (4096, 640, 640, True), (5, 8, 4, True),
]
CONV = [  # N, C, H, W, K, ksize, stride, pad, bias: the shapes of tests/test_f16_gpu.py
    (1, 4, 32, 32, 320, 3, 1, 1, True), (1, 320, 32, 32, 4, 3, 1, 1, True), (2, 320, 24, 24, 320, 3, 1, 1, True),
    (1, 640, 16, 16, 320, 1, 1, 0, True), (2, 64, 13, 11, 72, 3, 2, 1, False), (1, 128, 5, 5, 64, 3, 1, 1, True),
    (3, 8, 7, 9, 12, 3, 1, 0, True),
]
GEMM = [(77, 320, 640), (203, 1232, 136), (1, 5120, 8), (130, 16, 4)]   # M, K, N


# ------------------------------------------------------------------------------------------ norm producers
# GroupNorm: integer data (|x| <= 8, one heavy element of 64) -- every group's sum s and sum of squares q is an integer
# below 2^24, hence an exact FP32 number in ANY summation order, and the output bits follow from the kernel's
# order-free tail alone (csrc/fused_norm.hip gn_finalize_tail and the apply pass), restated here in numpy float32:
#   mean = s / cnt;  var = max(fma(-mean, mean, q / cnt), 0);  rstd = 1 / sqrt(var + eps)
#   a = rstd * gamma;  b = fma(-mean, a, beta);  y = f16(fma(x, a, b))
# A dropped, doubled or mis-grouped element changes an integer, and with it the bits.
HEAVY = 64.0
GN_EPS = np.float32(1e-5)


def fma32(a, b, c):
    """Correctly rounded FP32 a * b + c (numpy has no fma): the product is exact in float64 (24 x 24 bits), the
    float64 sum is rounded to odd with the exact error of the two-sum, and 53 >= 24 + 2 bits make the final rounding
    to FP32 the single rounding of the exact value."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.copy().view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    away = (err > 0) == (s > 0)                    # the exact value lies beyond s, away from zero
    bits = np.where(fix, bits + np.where(away, 1, -1), bits)
    return bits.view(np.float64).astype(np.float32)


def gn_group_sums(x, G):
    """Exact int64 (s, q) per (image, group) of integer-valued x [N, HW, C]."""
    N, HW, C = x.shape
    xi = x.astype(np.int64)
    assert np.array_equal(xi.astype(np.float16), x), "not integer-valued"
    v = xi.reshape(N, HW, G, C // G)
    return v.sum(axis=(1, 3)), (v * v).sum(axis=(1, 3))


def gn_expected(x, gamma, beta, G, eps=GN_EPS):
    """The pre-activation FP16 bits of GroupNorm on integer-valued x [N, HW, C], from the closed formula."""
    N, HW, C = x.shape
    cg = C // G
    s, q = gn_group_sums(x, G)
    cnt = HW * cg
    assert cnt < 2 ** 24 and np.abs(s).max() < 2 ** 24 and q.max() < 2 ** 24, "sums not exact in FP32"
    cntf = np.float32(cnt)
    mean = s.astype(np.float32) / cntf
    var = np.maximum(fma32(-mean, mean, q.astype(np.float32) / cntf), np.float32(0))
    rstd = np.float32(1) / np.sqrt(var + np.float32(eps), dtype=np.float32)
    mean_c, rstd_c = np.repeat(mean, cg, axis=1), np.repeat(rstd, cg, axis=1)          # [N, C]
    a = rstd_c * gamma.astype(np.float32)[None]
    b = fma32(-mean_c, a, beta.astype(np.float32)[None])
    y = fma32(x.astype(np.float32), a[:, None, :], b[:, None, :])
    return y.astype(np.float16), dict(s=s, q=q, mean=mean, var=var, rstd=rstd)


def _seeded_affine(seed, C):
    gamma = (dd.normal_f16(seed, (C,), 0.3).astype(np.float32) + 1).astype(np.float16)
    return gamma, dd.normal_f16(seed + 1, (C,), 0.2)


@functools.lru_cache(maxsize=64)
def gn_base(N, HW, C, G, seed=0):
    """Integers in [-8, 8]; group 1 of the last image is constant (variance exactly 0) and, where there is more
    than one image, image 0 is all zero."""
    s0 = _seed(N, HW, C, G, seed, 91)
    x = dd.int8(s0, (N, HW, C), -8, 9).astype(np.float16)
    cg = C // G
    if G > 1:
        x[N - 1, :, cg:2 * cg] = 3.0
    if N > 1:
        x[0] = 0
    gamma, beta = _seeded_affine(s0 + 1, C)
    x.setflags(write=False)
    return x, gamma, beta


def gn_heavy_positions(geom, C1=None):
    """{name: (pixel, channel)} of the single heavy element: first / last pixel of the image, of a chunk, the first
    pixel of the last chunk, the last pixel lane of a block iteration; first / last channel of a group, both ends of
    an octet that straddles two groups; with two sources the last channel of x and the first of x2.  `geom`: a
    tests/norm_edges.py gn_launch() dict."""
    HW, C, cg, PP, ppb, nchunk = (geom[k] for k in ("HW", "C", "cg", "PP", "ppb", "nchunk"))
    G = C // cg
    gm = min(G - 1, max(2, G // 2))                            # a middle group (not the constant one)
    c0 = gm * cg
    pos = {"first_pixel": (0, c0 + 1), "last_pixel": (HW - 1, c0 + 1)}
    k = 1 if nchunk > 2 else 0                                 # a chunk that is neither first nor last where one exists
    pos["chunk_first"] = (min(k * ppb, HW - 1), c0)
    pos["chunk_last"] = (min((k + 1) * ppb, HW) - 1, c0)
    pos["last_chunk_first"] = ((nchunk - 1) * ppb, c0 + cg - 1)
    pos["last_pixel_lane"] = (min(k * ppb + PP, HW) - 1, c0 + cg - 1)
    pos["group_first_channel"] = (HW // 2, c0)
    pos["group_last_channel"] = (HW // 2, c0 + cg - 1)
    for o in range(C // 8):
        if (8 * o) // cg != (8 * o + 7) // cg and (8 * o) // cg >= 2:
            pos["octet_leading_half"] = (HW // 2, 8 * o)
            pos["octet_trailing_half"] = (HW // 2, 8 * o + 7)
            pos["octet_boundary_below"] = (HW // 3, ((8 * o + 7) // cg) * cg - 1)
            pos["octet_boundary_above"] = (HW // 3, ((8 * o + 7) // cg) * cg)
            break
    if C1 is not None and C1 != C:
        pos["x_last_channel"] = (HW - 1, C1 - 1)
        pos["x2_first_channel"] = (0, C1)
    return pos


def gn_heavy(N, HW, C, G, pixel, channel, seed=0):
    """The base tensor with x[N - 1, pixel, channel] = 64, and the (image, group) whose sums that changes."""
    x, gamma, beta = gn_base(N, HW, C, G, seed)
    x = x.copy()
    old = int(x[N - 1, pixel, channel])
    x[N - 1, pixel, channel] = HEAVY
    return x, gamma, beta, dict(image=N - 1, group=channel // (C // G), ds=int(HEAVY) - old,
                                dq=int(HEAVY) ** 2 - old * old)


# LayerNorm: rows of small integers in which every 16-column group sums to zero.  Every group mean, unit mean and the
# row mean are exactly 0, every partial of the centred sums of squares is an exact integer, and the bits follow from
#   var = f32(Q) * rn(1 / C);  rstd = 1 / sqrt(var + eps);  y = f16(fma(x * rstd, gamma, beta))
def ln_zero_sum_rows(M, C, seed=0):
    assert C % 16 == 0
    half = dd.int8(_seed(M, C, seed, 92), (M, C // 16, 8), -8, 9).astype(np.int64)
    g = np.concatenate([half, -half], axis=2)                                   # [M, C / 16, 16]: sums to zero
    order = np.argsort(dd.u64(_seed(M, C, seed, 93), M * (C // 16) * 16).reshape(M, C // 16, 16), axis=2, kind="stable")
    x = np.take_along_axis(g, order, axis=2).reshape(M, C)
    assert (x.reshape(M, -1, 16).sum(axis=2) == 0).all()
    return x.astype(np.float16)


def ln_expected_zero_mean(x, gamma, beta, eps=GN_EPS):
    """Bits of LayerNorm on rows whose 16-column groups all sum to zero (asserted)."""
    M, C = x.shape
    xi = x.astype(np.int64)
    assert np.array_equal(xi.astype(np.float16), x) and (xi.reshape(M, -1, 16).sum(axis=2) == 0).all()
    Q = (xi * xi).sum(axis=1)
    assert Q.max() < 2 ** 24
    inv_c = np.float32(1) / np.float32(C)
    var = Q.astype(np.float32) * inv_c
    rstd = np.float32(1) / np.sqrt(var + np.float32(eps), dtype=np.float32)
    nrm = x.astype(np.float32) * rstd[:, None]
    return fma32(nrm, gamma.astype(np.float32)[None], beta.astype(np.float32)[None]).astype(np.float16)


def ln_expected_constant(c, C, gamma, beta, eps=GN_EPS):
    """Bits of LayerNorm on a row of C copies of the small integer c: every sum is an exact integer and every unit
    holds the same values, so the statistics are order-free; rn(1 / C) makes mean differ from c by a rounding unless C
    is a power of two, and the formula carries that through."""
    G = C // 16
    U = 1
    while U < 16 and G % (2 * U) == 0:
        U *= 2
    per = G // U
    f = np.float32
    inv_nu, inv_c = f(1) / f(16 * per), f(1) / f(C)
    assert abs(C * c) < 2 ** 24
    mean = f(C * c) * inv_c
    mu = f(16 * per * c) * inv_nu
    e = mu - mean
    du = fma32(e * f(16 * per), e, f(0))                       # M2 of a constant unit is 0
    var = f(U) * du * inv_c                                    # U equal values through the tree: an exact product
    rstd = f(1) / np.sqrt(var + f(eps), dtype=np.float32)
    nrm = (f(c) - mean) * rstd
    return fma32(np.full(C, nrm, np.float32), gamma.astype(np.float32), beta.astype(np.float32)).astype(np.float16)


def ln_heavy_columns(C):
    """Columns the heavy element visits: first and last, both sides of every 16-column group boundary of one unit,
    a unit boundary, and the lane-63 -> lane-0 chunk wrap (columns 504 .. 519) where the row is that long."""
    G = C // 16
    U = 1
    while U < 16 and G % (2 * U) == 0:
        U *= 2
    per = G // U
    u = U // 2                                                 # a middle unit
    cols = {0, C - 1}
    for k in range(per + 1):
        b = 16 * (u * per + k)                                 # k = 0 and k = per: the unit's own boundaries
        cols |= {b - 1, b}
    if C >= 1024:
        cols |= set(range(504, 520))
    return sorted(c for c in cols if 0 <= c < C)


@functools.lru_cache(maxsize=32)
def ln_heavy(C, seed=0):
    """Row 0: the zero-sum base row; row 1 + i: the base row with column ln_heavy_columns(C)[i] set to 64."""
    cols = ln_heavy_columns(C)
    base = ln_zero_sum_rows(1, C, seed)
    x = np.repeat(base, 1 + len(cols), axis=0)
    for i, c in enumerate(cols):
        x[1 + i, c] = HEAVY
    gamma, beta = _seeded_affine(_seed(C, seed, 94), C)
    return x, gamma, beta, cols


# Quantizer edges through the producers: FP16 values v = k / 8 in [-80, 80] -- with scale_inv 2 or 4 and zero points
# on the quarter grid, v * scale_inv + zero_point lands exactly on integers, on k + 0.5 ties (both parities of k) and
# beyond both clamp ends.
QEDGE_LN = ((2.0, 0.0), (4.0, -3.0), (4.0, 100.5))            # one (scale_inv, zero_point) per LayerNorm slot
QEDGE_GN, QEDGE_RAW = (2.0, 0.5), ((2.0, 0.0), (4.0, 27.5))


def qedge_values(n, seed=0):
    k = np.arange(-640, 641)
    v = (k[dd.u64(_seed(n, seed, 95), n) % np.uint64(k.size)].astype(np.float64) / 8)
    v[:k.size] = (k / 8)[:min(n, k.size)] if n >= k.size else v[:k.size]
    return v.astype(np.float16)


def qedge_facts(v, s_inv, zp):
    """What a value set reaches under one quantizer: ties to both parities, both clamps, values beyond them."""
    t = v.astype(np.float64) * s_inv + zp
    tie = (t - np.floor(t)) == 0.5
    inside = (t > -128) & (t < 127)
    return dict(tie_even=bool((tie & inside & (np.floor(t) % 2 == 0)).any()),
                tie_odd=bool((tie & inside & (np.floor(t) % 2 == 1)).any()),
                at_low=bool((np.abs(t + 128) <= 0.5).any()), at_high=bool((np.abs(t - 127) <= 0.5).any()),
                below=bool((t < -129).any()), above=bool((t > 128).any()))
