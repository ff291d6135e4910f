"""Operands whose INT32 accumulators FP32 cannot hold (tests/test_heavy_acc_gpu.py runs them on every INT8
launch, tests/test_heavy_acc_host.py checks the operands and the references on the CPU).

Every INT8 epilogue starts with f32(acc), round to nearest even (oracle/mixdq_oracle.c); |acc| >= 2^24 is in
general no FP32 number.  The operands here are a tensor resting at its zero point: a = -128 everywhere but at a few
reserved k, where it lies d in {1, 3, 5} above; zp = -128, so bias0 = -128 * wsum is a multiple of 128 and exact.
Then acc = base + delta with base = -128 * wsum huge and delta = sum d * w small, and with scale 1 and no bias the one
correct output is the integer RNE(acc) - base: a conversion that truncates, or rounds halves away, is off by one
FP32 spacing (2, 4 or 8) in a known share of the outputs, not once in 2^12.

Linear: output column n is of class n % 8, set by how many of its weights sit on a rail:

  0  k0 at qmin      base just above +2^24        4  k0 at qmin      just above +2^26
  1  k0 at qmax      just below -2^24             5  none            the control: every accumulator exact
  2  k0 at qmin      just above +2^25             6  2^24 / (128 |qmin|) at qmin: base exactly 2^24
  3  k0 at qmax      just below -2^25             7  every free k at qmin: as large as K allows

k0 = target // (128 |q|) + 1 (INT8: 1025, 1033, 2049, 2065, 4097).  Where K cannot hold a class's k0 (packed W4 /
W2: qmin = -8 / -2, k0 16 / 64 times larger) the class takes the 2^24 target of its sign, and where that does not
fit either, class 0's.  The k with k % 64 == 5 are reserved: they carry ordinary weights in every column, and the
raised activations sit on them only, so |delta| <= P * 5 * 3 = 120 -- inside the INT8 range the GEMM + GEGLU output
needs, and far inside the 2047 up to which RNE(acc) - base is an FP16 number.  The heavy k of column n are the free
k number (STRIDE * j + n) % free, j < k0: spread over every K-tile.  The other weights lie in [-3, 3] (W2: [-1, 1])
and sum to zero, so base is the rail weights' share alone.

The expectation is integer arithmetic throughout: delta by gathering the reserved weights, nearest-even to the FP32
spacing at |acc| with shifts, the FP16 bit pattern of the (exactly representable) difference assembled from its bits.

Conv (3x3, stride 1, pad 1, C = 256: nine taps of 256; interior windows reach 3.8e7, edges 2.5e7, and the corners of
an all -128 filter land exactly on 2^24): the same, output channel classes by k % 8, the expectation per pixel by
window intersection (the taps inside the image), as tests/conv_geometry.py does.

A second operand set keeps the accumulators and exercises the FP16 end: per-column scales (a non-power-of-two one,
2^-20, one that puts outputs on both sides of 65504 / 65520 / inf, one among the FP16 subnormals), an FP16 bias and
integer residuals.  Its expectation is the C oracle's.

Imports without a GPU and without the built library.
"""
import functools
import math
import os

import numpy as np

from tests import tile_edges as te

ZP = -128
P = 8                       # raised activations per row
STEPS = (1, 3, 5)           # how far above -128 (odd: delta's parity is the weights')
REST = 3                    # |ordinary weight| <= REST
DELTA_MAX = P * max(STEPS) * REST
RESERVED_EVERY, RESERVED_AT = 64, 5
K_INT8, K_W4, K_W2 = 4224, 19200, 66688       # 33, 150 and 521 K-tiles of 128
TARGETS = {0: (1 << 24, -1), 1: (1 << 24, +1), 2: (1 << 25, -1), 3: (1 << 25, +1), 4: (1 << 26, -1)}   # rail: -1 qmin
QMAX = {-128: 127, -8: 7, -2: 1}


# ------------------------------------------------------------------------------------ integer arithmetic
def _shift_of(mag):
    """FP32 spacing at |acc| as a shift: 0 below 2^24, then 1, 2, ... (|acc| < 2^31)."""
    s = np.zeros(mag.shape, dtype=np.int64)
    for k in range(24, 31):
        s += mag >= (1 << k)
    return s


def round_f32(acc, mode="rne"):
    """The integer f32(acc) stands for: `acc` (int64, |acc| < 2^31) rounded to the FP32 spacing at its magnitude --
    nearest, ties to the even multiple ("rne": the specification); toward zero ("rtz") and nearest with ties away
    ("rha") are the wrong conversions the tests must tell from it.  No float is involved."""
    acc = np.asarray(acc, dtype=np.int64)
    mag = np.abs(acc)
    assert int(mag.max(initial=0)) < 1 << 31
    s = _shift_of(mag)
    q, rem, half = mag >> s, mag & ((1 << s) - 1), (1 << s) >> 1
    if mode == "rne":
        up = (rem > half) | ((rem == half) & (s > 0) & ((q & 1) == 1))
    elif mode == "rha":
        up = (rem >= half) & (s > 0)
    else:
        assert mode == "rtz"
        up = np.zeros(mag.shape, dtype=bool)
    return np.where(acc < 0, -1, 1) * ((q + up) << s)


def inexact(acc):
    acc = np.asarray(acc, dtype=np.int64)
    mag = np.abs(acc)
    return (mag & ((1 << _shift_of(mag)) - 1)) != 0


def tie(acc):
    acc = np.asarray(acc, dtype=np.int64)
    mag = np.abs(acc)
    s = _shift_of(mag)
    return (s > 0) & ((mag & ((1 << s) - 1)) == ((1 << s) >> 1))


def f16_bits(v):
    """FP16 bit patterns (uint16) of integers that FP16 holds exactly (asserted), assembled from their bits."""
    v = np.asarray(v, dtype=np.int64)
    mag = np.abs(v)
    assert int(mag.max(initial=0)) < 1 << 16
    e = np.zeros(v.shape, dtype=np.int64)
    for k in range(1, 16):
        e += mag >= (1 << k)
    down = np.maximum(e - 10, 0)
    assert not (mag & ((1 << down) - 1)).any(), "an expectation is no FP16 number"
    mant = (mag >> down) << np.maximum(10 - e, 0)          # 1.m with the leading one at bit 10
    bits = np.where(mag == 0, 0, ((e + 15) << 10) + (mant - 1024)) + np.where(v < 0, 0x8000, 0)
    return bits.astype(np.uint16)


# ---------------------------------------------------------------------------------------------- linear
def _stride(free):
    return next(s for s in (37, 41, 43, 47, 53) if math.gcd(s, free) == 1)


def _k0(cls, K_free, qmin):
    """(count, rail value) of a column class."""
    qmax = QMAX[qmin]
    if cls == 5:
        return 0, qmin
    if cls == 6:
        return (1 << 24) // (128 * -qmin), qmin
    if cls == 7:
        return K_free, qmin
    target, rail = TARGETS[cls]
    for tgt, r in ((target, rail), (1 << 24, rail), (1 << 24, -1)):
        q = qmin if r < 0 else qmax
        k0 = tgt // (128 * abs(q)) + 1
        if k0 <= K_free:
            return k0, q
    raise AssertionError("K too short for 2^24")


def negative_reachable(K, qmin):
    """Can a column of K weights at qmax pass -2^24?  (W2: only past K = 131072, where an all-qmin column's x64
    accumulator passes 2^31; its cases have the positive side only.)"""
    free = K - len(range(RESERVED_AT, K, RESERVED_EVERY))
    return (1 << 24) // (128 * QMAX[qmin]) + 1 <= free


def heavy_weights(N, K, qmin, seed, classes=None):
    """int8 [N, K] and the per-column class.  `classes`: the class of each column (default n % 8)."""
    reserved = np.arange(RESERVED_AT, K, RESERVED_EVERY)
    free = np.setdiff1d(np.arange(K), reserved)
    nf = free.size
    st = _stride(nf)
    cls = np.arange(N) % 8 if classes is None else np.asarray(classes)
    rng = np.random.default_rng(seed)
    lim = min(REST, QMAX[qmin])
    w = np.empty((N, K), dtype=np.int8)
    j = np.arange(nf)
    for n in range(N):
        k0, q = _k0(int(cls[n]), nf, qmin)
        rest_n = K - k0
        r = rng.integers(-lim, lim + 1, rest_n // 2)
        rest = np.concatenate([r, -r, np.zeros(rest_n % 2, dtype=np.int64)])          # sums to zero
        order = np.concatenate([free[(st * j + n) % nf], reserved])                   # a permutation of range(K)
        vals = np.concatenate([np.full(k0, q, dtype=np.int64), rng.permutation(rest)])
        w[n, order] = vals
    return w, cls, reserved


def heavy_activations(M, K, reserved):
    """int8 [M, K] at -128 with P reserved k per row raised by STEPS[m % 3]; the positions and the steps."""
    a = np.full((M, K), -128, dtype=np.int8)
    nr = reserved.size
    assert nr >= P
    pos = reserved[(np.arange(M)[:, None] * 3 + np.arange(P)[None, :] * (nr // P)) % nr]     # [M, P], distinct per row
    d = np.asarray(STEPS)[np.arange(M) % len(STEPS)]
    np.put_along_axis(a, pos, (-128 + d)[:, None].astype(np.int8).repeat(P, 1), axis=1)
    return a, pos, d


class Linear:
    """One linear problem: a [M, K], w [N, K] int8; bias0, scale f32; acc, base, delta int64; want uint16 (FP16 bits of
    RNE(acc) - base); cls [N]."""


@functools.lru_cache(maxsize=None)
def linear(M, N, K, qmin=-128, geglu=False):
    """`geglu`: N = 2 D value|gate columns in the ordinary [2D, K] row order (values 0 .. D-1 of class n % 8, gates
    D .. 2D-1 all zero with bias 16)."""
    c = Linear()
    c.M, c.N, c.K, c.qmin = M, N, K, qmin
    D = N // 2 if geglu else N
    w, cls, reserved = heavy_weights(D, K, qmin, seed=K + 31 * N + 7 * qmin)
    a, pos, d = heavy_activations(M, K, reserved)
    wsum = w.sum(axis=1, dtype=np.int64)
    c.base = (-128 * wsum)[None, :]                                                   # [1, D]
    c.delta = (w.astype(np.int64)[:, pos] * d[None, :, None]).sum(axis=2).T          # [M, D]: sum_j d w[n, pos[m, j]]
    assert int(np.abs(c.delta).max()) <= DELTA_MAX
    c.acc = c.base + c.delta
    c.cls = cls
    c.want_int = round_f32(c.acc) - c.base
    c.want = f16_bits(c.want_int)
    c.bias0 = (wsum * ZP).astype(np.float32)
    assert np.array_equal(c.bias0.astype(np.int64), -128 * wsum)                      # (a check, not the expectation)
    if geglu:
        assert int(np.abs(c.want_int).max()) <= 127
        w = np.concatenate([w, np.zeros((D, K), dtype=np.int8)])
        c.bias0 = np.concatenate([c.bias0, np.zeros(D, dtype=np.float32)])
        c.bias = np.concatenate([np.zeros(D), np.full(D, 16.0)]).astype(np.float16)
        c.want_q = c.want_int.astype(np.int8)
    c.a, c.w = a, w
    c.scale = np.ones(N, dtype=np.float32)
    return c


def wrong(c, mode):
    """What a conversion of `mode` ("rtz", "rha") would give in place of c.want_int."""
    return round_f32(c.acc, mode) - c.base


# ------------------------------------------------------------------------------- the FP16 end (second set)
SCALE_CLASSES = ("order1", "pow2", "overflow", "subnormal")
SCALES = {"order1": np.float32(0.0137), "pow2": np.float32(2.0 ** -20), "overflow": np.float32(4095.0),
          "subnormal": np.float32(3 * 2.0 ** -27)}


def fp16_end(c, seed=5):
    """(scale [N] f32, bias [N] f16, residual [M, N] f16 of integers, scale class per column): columns n with
    (n // 8) % 4 == i take SCALES[SCALE_CLASSES[i]] -- every accumulator class meets every scale class.  4095 * 16
    = 65520, the first value that rounds to inf (a bias below zero brings it back to 65504), and 4095 * 15 stays finite; 3 * 2^-27 * delta lies
    among the FP16 subnormals (multiples of 2^-24), where the bias is a subnormal too."""
    N = c.cls.size
    rng = np.random.default_rng(seed + N)
    sclass = (np.arange(N) // 8) % 4
    scale = np.asarray([SCALES[SCALE_CLASSES[i]] for i in sclass], dtype=np.float32)
    bias = rng.uniform(-1, 1, N).astype(np.float16)
    sub = sclass == 3
    bias[sub] = (rng.integers(-5, 6, int(sub.sum())) * 2.0 ** -24).astype(np.float16)
    residual = rng.integers(-64, 65, (c.acc.shape[0], N)).astype(np.float16)
    return scale, bias, residual, sclass


# ------------------------------------------------------------------------------------------------ conv
CONV_C, CONV_W4_C = 256, 3072
# class -> (target, taps that reach it, rail): 9 taps = interior windows, 6 = edge windows
CONV_TARGETS = {0: (1 << 24, 9, -1), 1: (1 << 24, 9, +1), 2: (1 << 25, 9, -1), 3: (1 << 25, 9, +1), 4: (1 << 24, 6, -1)}


def _conv_count(cls, C, n_free, qmin):
    """(rail weights per tap, rail value): INT8 at C = 256 -- 114, 115, 228, 230, 171; 0; all 256 channels (the
    corners of that filter land exactly on 2^24); all free channels."""
    qmax = QMAX[qmin]
    if cls == 5:
        return 0, qmin
    if cls == 6:
        return C, qmin
    if cls == 7:
        return n_free, qmin
    target, taps, rail = CONV_TARGETS[cls]
    for tgt, tp, r in ((target, taps, rail), (1 << 24, 9, rail), (1 << 24, 9, -1)):
        q = qmin if r < 0 else qmax
        cnt = tgt // (tp * 128 * abs(q)) + 1
        if cnt <= n_free:
            return cnt, q
    raise AssertionError("C too small for 2^24")


class Conv:
    """x [n, H, W, C], w [K, 3, 3, C] int8; wsum f32 [K, 3, 3]; acc, base, delta int64 [n, H, W, K]; want uint16."""


def _taps(H, W):
    """(r, s, output rows, output columns, input rows, input columns) of the taps of a 3x3 / pad 1 window that lie
    inside the image: output pixel (h, w) reads input (h + r - 1, w + s - 1)."""
    for r in range(3):
        for s in range(3):
            h0, h1 = max(0, 1 - r), min(H, H + 1 - r)
            w0, w1 = max(0, 1 - s), min(W, W + 1 - s)
            yield r, s, slice(h0, h1), slice(w0, w1), slice(h0 + r - 1, h1 + r - 1), slice(w0 + s - 1, w1 + s - 1)


@functools.lru_cache(maxsize=None)
def conv(n, H, W, C, K, qmin=-128, ups=False):
    """`ups`: the image is the nearest 2x upsampling of c.x_small [n, H / 2, W / 2, C] (the upsample fold).  Packed W4 (qmin = -8) needs C = 3072 to pass 2^24 on both sides; classes it cannot reach take the 2^24 target."""
    c = Conv()
    c.n, c.H, c.W, c.C, c.K, c.qmin = n, H, W, C, K, qmin
    reserved = np.arange(RESERVED_AT, C, RESERVED_EVERY)
    free = np.setdiff1d(np.arange(C), reserved)
    st = _stride(free.size)
    rng = np.random.default_rng(C + 31 * K)
    lim = min(REST, QMAX[qmin])
    w = rng.integers(-lim, lim + 1, (K, 3, 3, C)).astype(np.int8)
    cls = np.arange(K) % 8
    for k in range(K):
        cnt, q = _conv_count(int(cls[k]), C, free.size, qmin)
        for tap in range(9):
            if cnt == C:
                w[k, tap // 3, tap % 3, :] = q
            else:
                w[k, tap // 3, tap % 3, free[(st * np.arange(cnt) + k + 5 * tap) % free.size]] = q
    # every pixel raises one reserved channel
    x = np.full((n, H, W, C), -128, dtype=np.int8)
    if ups:
        pix = np.arange(n * H * W // 4).reshape(n, H // 2, W // 2).repeat(2, axis=1).repeat(2, axis=2)
    else:
        pix = np.arange(n * H * W).reshape(n, H, W)
    ch = reserved[pix % reserved.size]
    d = np.asarray(STEPS)[(pix // reserved.size + pix) % len(STEPS)]
    np.put_along_axis(x, ch[..., None], (-128 + d)[..., None].astype(np.int8), axis=3)
    wsum = w.sum(axis=3, dtype=np.int64)                                              # [K, 3, 3]
    base = np.zeros((n, H, W, K), dtype=np.int64)
    delta = np.zeros((n, H, W, K), dtype=np.int64)
    wl = w.astype(np.int64)
    for r, s, oh, ow, ih, iw in _taps(H, W):
        base[:, oh, ow, :] += -128 * wsum[:, r, s]
        delta[:, oh, ow, :] += wl[:, r, s, :].T[ch[:, ih, iw]] * d[:, ih, iw, None]   # w[k, r, s, ch(pixel)] * d(pixel)
    plain = cls != 6                                                                  # (class 6: multiples of 128)
    assert int(np.abs(delta[..., plain]).max()) <= 9 * max(STEPS) * REST
    c.x, c.w, c.cls = x, w, cls
    c.x_small = np.ascontiguousarray(x[:, ::2, ::2]) if ups else None
    c.wsum = wsum.astype(np.float32)
    c.base, c.delta, c.acc = base, delta, base + delta
    c.want_int = round_f32(c.acc) - base
    c.want = f16_bits(c.want_int)
    c.scale = np.ones(K, dtype=np.float32)
    return c


# ------------------------------------------------------------------------------------------- the cases
def int8_tiles():
    return sorted(te.IGEMM)


def gemm_shape(cfg):
    """M = BM + 1, N = BN + 4, K = 4224: two row tiles, an N tail in the second column tile, 33 (BK = 128) or 66
    K-tiles."""
    bm, bn, bk, st = te.tile(cfg)
    return bm + 1, bn + 4, K_INT8


PERSISTENT = 71             # csrc/igemm_pp.h pp_ok: its FP16 rows leave in 16-byte pieces -- N % 8 == 0, else 70's kernel runs


def gemm_shapes(cfg):
    """gemm_shape(cfg), and for the persistent kernel the N = BN + 8 at which it runs itself."""
    M, N, K = gemm_shape(cfg)
    return [(M, N, K)] + ([(M, N + 4, K)] if cfg == PERSISTENT else [])


def grouped_shapes(cfg):
    """The members of one grouped launch: N = BN - 4, BN + 4, 2 BN + 4 on the same activations."""
    bm, bn, bk, st = te.tile(cfg, te.GROUPED)
    return [(bm + 1, n, K_INT8) for n in (bn - 4, bn + 4, 2 * bn + 4)]


def geglu_shape(cfg):
    bm, bn, bk, st = te.tile(cfg)
    return bm + 1, bn + 32, K_INT8


def packed_tiles(bits):
    """Two admissible tiles of a packed width: the smallest and the largest tile area."""
    ok = [c for c in sorted(te.IGEMM) if bits == 4 or te.w2_admissible(c)]
    area = lambda c: te.tile(c)[0] * te.tile(c)[1]
    return sorted({min(ok, key=area), max(ok, key=area)})


HALO = te._xmacro(os.path.join(te.CSRC, "iconv.h"), "MIXDQ_HALO_TILES")     # id -> (TH, TW, BN, CK, WNG)
CONV_SHAPE = (2, 16, 16)                 # n, H, W: one 16 x 16 patch (or four of 8 x 8) per image, every border class
CONV_W4_SHAPE = (1, 16, 16)              # at C = 3072
GENERIC_CONV = (1, 8, 8, 248, 16)        # C % 16 != 0, R S C = 2232: the one-output-per-thread kernel
GENERIC_LINEAR = (17, 72, K_INT8 + 4)    # K % 16 != 0
LN_TILES = (44, 45, 56)                  # csrc/igemm_ln.hip; N = 640: eight 80-column tiles, one LayerNorm unit each
LN_N = 640


def conv_k(bn):
    return bn + 8


def host_linear_cases():
    """The distinct linear problems the GPU file runs, as linear()'s arguments."""
    out = {shape + (-128, False) for cfg in int8_tiles() for shape in gemm_shapes(cfg)}
    out |= {geglu_shape(cfg) + (-128, True) for cfg in int8_tiles() if te.geglu_admissible(cfg)}
    out |= {GENERIC_LINEAR + (-128, False)}
    out |= {shape + (-128, False) for cfg in te.GROUPED for shape in grouped_shapes(cfg)}
    out |= {(te.tile(cfg)[0] + 1, LN_N, K_INT8, -128, False) for cfg in LN_TILES}
    for bits, qmin, K in ((4, -8, K_W4), (2, -2, K_W2)):
        out |= {(5, te.tile(cfg)[1] + 4, K, qmin, False) for cfg in packed_tiles(bits)}
    out.add((5, 96, K_W4, -8, True))
    return sorted(out)


def host_conv_cases():
    """The distinct conv problems the GPU file runs, as conv()'s arguments."""
    out = {CONV_SHAPE + (CONV_C, conv_k(te.tile(cfg)[1]), -128) for cfg in int8_tiles()}
    out |= {CONV_SHAPE + (CONV_C, conv_k(row[2]), -128) for row in HALO.values()}
    out |= {CONV_W4_SHAPE + (CONV_W4_C, conv_k(row[2]), -8) for row in HALO.values()}
    out.add(GENERIC_CONV + (-128,))
    return sorted(out)


def all_conv_cases():
    """host_conv_cases() and the upsampled image of the fold (conv()'s arguments)."""
    return host_conv_cases() + [CONV_SHAPE + (CONV_C, conv_k(row[2]), -128, True) for row in HALO.values()][:1]
