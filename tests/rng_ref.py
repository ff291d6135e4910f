"""The device-side Gaussian noise (include/mixdq_math.h: mixdq_philox4x32_10, mixdq_rng_*) restated in numpy, operation
for operation: Philox4x32-10 in uint32 / uint64 integer arithmetic, the two Box-Muller pairs in float32 with every
rounding its own ufunc call and every fused multiply-add through tests/exact_inputs.fma32 (numpy has none)."""
import numpy as np

from tests.exact_inputs import fma32

f32 = np.float32
u32 = np.uint32
u64 = np.uint64
STREAM_START, STREAM_STEP, STREAM_VAE = 0, 1, 2     # include/mixdq_hip.h MIXDQ_RNG_STREAM_*
M0, M1 = u64(0xD2511F53), u64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = u64(0xFFFFFFFF)
_CHUNK = 1 << 18                                    # fma32 makes a dozen float64 temporaries: keep them in cache


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars), key: two -> four uint32 arrays."""
    c = [np.asarray(v, dtype=u64) & MASK32 for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(v, dtype=u64) & MASK32 for v in key)
    for rnd in range(10):
        p0 = M0 * c[0]                               # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = M1 * c[2]
        c = [(p1 >> u64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> u64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0 = (k0 + u64(W0)) & MASK32
        k1 = (k1 + u64(W1)) & MASK32
    return [v.astype(u32) for v in c]


def _chunked(fn, *arrays):
    arrays = [np.atleast_1d(a) for a in arrays]
    n = arrays[0].size
    if n <= _CHUNK:
        return fn(*arrays)
    parts = [fn(*(a[i:i + _CHUNK] for a in arrays)) for i in range(0, n, _CHUNK)]
    if isinstance(parts[0], tuple):
        return tuple(np.concatenate([p[j] for p in parts]) for j in range(len(parts[0])))
    return np.concatenate(parts)


def _log_u24(k):
    x = k.astype(f32)                                # exact: k <= 2^24
    bits = x.view(u32)
    e = (bits - u32(0x3F2AAAAB)) & u32(0xFF800000)
    m = (bits - e).view(f32)                         # in [2/3, 4/3)
    i = ((e.view(np.int32) >> 23) - np.int32(24)).astype(f32)
    m = m - f32(1.0)
    s = m * m
    r = np.full_like(m, f32(-0.130310059))
    t = np.full_like(m, f32(0.140869141))
    r = fma32(r, s, f32(-0.121483512))
    t = fma32(t, s, f32(0.139814854))
    r = fma32(r, s, f32(-0.166846126))
    t = fma32(t, s, f32(0.200120345))
    r = fma32(r, s, f32(-0.249996200))
    r = fma32(t, m, r)
    r = fma32(r, m, f32(0.333331972))
    r = fma32(r, m, f32(-0.5))
    r = fma32(r, s, m)
    return fma32(i, f32(0.693147182), r)


def log_u24(k):
    """mixdq_rng_log_u24: log(k * 2^-24) for k = 1 .. 2^24 (uint32 array) -> float32."""
    return _chunked(_log_u24, np.asarray(k, dtype=u32))


def _sincos_u24(j):
    octant = j >> u32(21)
    r = j & u32(0x1FFFFF)
    r = np.where((octant & u32(1)) != 0, u32(0x200000) - r, r)
    x = r.astype(f32) * f32(2.0 ** -21)              # exact, in [0, 1]: the angle inside the octant is x * pi/4
    y = x * x
    q = fma32(np.full_like(x, f32(-3.595429006963968e-05)), y, f32(0.0024900068528950214))
    q = fma32(q, y, f32(-0.08074543625116348))
    w = fma32(q, y, f32(-2.4276526e-08))
    xw = x * w
    s = fma32(x, np.array(0x3F490FDB, dtype=u32).view(f32), xw)
    p = fma32(np.full_like(x, f32(3.541952764862799e-06)), y, f32(-0.00032596138771623373))
    p = fma32(p, y, f32(0.01585433818399906))
    p = fma32(p, y, f32(-0.3084251284599304))
    c = fma32(p, y, f32(1.0))
    swap = (((octant + u32(1)) >> u32(1)) & u32(1)) != 0
    sn = np.where(swap, c, s)
    cs = np.where(swap, s, c)
    sn = np.where(octant >= u32(4), -sn, sn)
    cs = np.where((((octant + u32(2)) >> u32(2)) & u32(1)) != 0, -cs, cs)
    return sn, cs


def sincos_u24(j):
    """mixdq_rng_sincos_u24: (sin, cos) of 2 pi j 2^-24 for j = 0 .. 2^24 - 1 (uint32 array) -> two float32 arrays."""
    return _chunked(_sincos_u24, np.asarray(j, dtype=u32))


def box_muller(ra, rb):
    """mixdq_rng_box_muller: two 32-bit words -> (z0, z1)."""
    ra, rb = np.asarray(ra, dtype=u32), np.asarray(rb, dtype=u32)
    lg = log_u24((ra >> u32(8)) + u32(1))
    rad = np.sqrt(f32(-2.0) * lg)
    sn, cs = sincos_u24(rb >> u32(8))
    return rad * cs, rad * sn


def normals_from_bits(r):
    """mixdq_rng_normals4 over a [n, 4] uint32 array -> [n, 4] float32."""
    r = np.asarray(r, dtype=u32).reshape(-1, 4)
    z0, z1 = box_muller(r[:, 0], r[:, 1])
    z2, z3 = box_muller(r[:, 2], r[:, 3])
    return np.stack([z0, z1, z2, z3], axis=1)


def randn_image(seed, n_image, stream=0, step=0):
    """One image's noise: float32 [n_image] in storage (NHWC) order, by the rule of include/mixdq_math.h."""
    seed = int(seed) & (2 ** 64 - 1)
    nq = (int(n_image) + 3) // 4
    q = np.arange(nq, dtype=u64)
    r = philox4x32_10((q & MASK32, q >> u64(32), u32(step), u32(stream)), (seed & 0xFFFFFFFF, seed >> 32))
    return normals_from_bits(np.stack(r, axis=1)).reshape(-1)[:n_image]


def randn(shape, seeds, stream=0, step=0):
    """_C.randn: [B, C, H, W] float32 (logical NCHW view of the NHWC values)."""
    B, Cc, H, W = shape
    out = np.stack([randn_image(s, Cc * H * W, stream, step) for s in seeds])
    return out.reshape(B, H, W, Cc).transpose(0, 3, 1, 2)


def ulp_error(got, exact):
    """|got - exact| in units of the float32 ulp at `exact` (float64 array); where exact == 0, got must be 0."""
    got = np.asarray(got, dtype=np.float64)
    exact = np.asarray(exact, dtype=np.float64)
    a = np.abs(exact)
    with np.errstate(divide="ignore"):
        ulp = np.exp2(np.floor(np.log2(np.where(a > 0, a, 1.0))) - 23.0)
    err = np.abs(got - exact) / ulp
    return np.where(a > 0, err, np.where(got == 0, 0.0, np.inf))
