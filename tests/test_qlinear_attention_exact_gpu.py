"""GPU tests of the fused to_q + cross-attention launch (mixdq_qlinear_w8a8_attn: the `if constexpr (ATT)` blocks of
csrc/igemm_kernel.h, a 64 x 128 x 128 tile with three stages that no GEMM tile list holds) on exact-result inputs.
Q comes out of the INT8 GEMM here, so the operands are built to make the GEMM produce a prescribed Q exactly
(tests/exact_inputs.py toq_operands(); checked on the CPU by tests/test_exact_inputs_host.py).

  a. selection      one-hot rows of `a` pick the hot key's sign code out of `w` (eight K-tiles): out[i] == v[j(i)] BIT
                    FOR BIT, INT8 / A4 outputs == quantize(v[j(i)]); W8, packed W4 and W2; k / v contiguous, column
                    slices of one k|v buffer, and k contiguous with v inside a wider, taller buffer (other row AND
                    batch strides).  Key counts 1, 4, 5, 63 .. 65, 77, 96, 97, 127, 128; 64 and 192 queries an image.
  b. counted once   q == 0 out of a GEMM whose every accumulator cancels: out == 2048 / tkv within one FP16 ulp (equal
                    at power-of-two counts); small-integer values at 1, 4, 64, 128 keys: fp16(sum / tkv) bit for bit.
  c. rescale        the staircases, the late dominant key and the equal scores of +-60 with q == 2 u out of the GEMM,
                    |v| up to 6e4 with a random-data Q, at 65 / 77 / 128 keys (two key tiles each): the tolerance of
                    tests/test_attention_gpu.py against the float64 oracle, finite, inside the range of the values, the
                    bits of attention_f16(to_q(a, w), k, v) in its tiled and its short-key form, a batch image equal
                    to its own launch.
  d. geometry       random data, the bits of the two-launch chain and the oracle's tolerance: 1, 2, 3, 4 and 8 K-tiles
                    against the three stages, five images of one M tile each, one and three N tiles, softmax scales
                    0.2 and 1 / 16, key counts on both sides of the half-wave mask split.
  e. refusals       more than 128 keys, T % 64, N % 128, K % 128, a key row stride off 8 elements, one of the two
                    quantizer scalars alone: the status, and a sentinel-filled output left as it was.

What (a) and (b) catch in this copy of the attention core, which a comparison with the stand-alone kernel cannot (the
two share the arithmetic): a K / V LDS-DMA piece in the wrong place or retired late against the K-tile pieces (eight
K-tiles: the pieces are seven tiles old) is another row; the clamped re-read of key tkv - 1 admitted past the mask
doubles its probe; the wave-private output staging written over the fp16 tile before every wave has read its Q
fragments gives queries that are no key.

Measured on an MI355X, (c), the largest error / (2e-3 + 4e-3 |ref|) of each kind over the three key counts, the fused
launch | attention_f16 on the same Q (each case prints its own, `-s`); the bits are equal, so are the figures:
    rise4 0.082 | 0.082 (3.4e-4)       rise40 0.077 | 0.077 (3.2e-4; at 65 keys the second tile's one key takes all: 5e-10)
    fall4 0.066 | 0.066 (2.0e-4)       fall40 0.060 | 0.060 (2.5e-4)
    late_dominant 0.000 | 0.000 (1.3e-14: the FP16 output is the dominant key's value row)
    equal_large 0.039 | 0.039, equal_large_negative 0.040 | 0.040 (1.2e-4)
    huge_values 0.107 | 0.107 (17.1 on results of 3e4 .. 6e4)
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import detdata as dd
from tests import exact_inputs as ei
from tests.test_attention_exact_gpu import S_INV, ZP, assert_bits, scal, t
from tests.test_attention_gpu import ATOL, RTOL
from tests.test_conv_geometry_gpu import ERR_ALIGNMENT, ERR_SHAPE, Buf, _p, _stream, _sync_status

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_INVALID_ARG = 1
WBITS = (8, 4, 2)
KV_LAYOUTS = ("contiguous", "packed", "mixed")
HEADS = ei.QATT_HEADS


def stored(w, wbits):
    """(device weight as the launch takes it, its keyword arguments)."""
    from mixdq_amd.nn.utils import pack_w2, pack_w4
    wt = torch.from_numpy(np.ascontiguousarray(w))
    return ((wt if wbits == 8 else pack_w4(wt) if wbits == 4 else pack_w2(wt)).to(DEV),
            dict(_w4=wbits == 4, _w2=wbits == 2))


def kv_views(k, v, layout, seed=0):
    """contiguous | packed: column slices of one [B, tkv, 2N] k|v buffer (row stride 2N, as the grouped k|v projection
    leaves them) | mixed: k contiguous, v rows 1 .. tkv and columns N .. 2N of a [B, tkv + 3, 3N] buffer of other
    numbers: k_row_stride != v_row_stride, and the batch strides differ by more than the row strides do."""
    B, tkv, N = k.shape
    if layout == "contiguous":
        return t(k), t(v)
    if layout == "packed":
        kv = t(np.concatenate([k, v], axis=-1))
        return kv[..., :N], kv[..., N:]
    wide = dd.normal_f16(9000 + seed, (B, tkv + 3, 3 * N), 300.0)
    wide[:, 1:tkv + 1, N:2 * N] = v
    vd = t(wide)[:, 1:tkv + 1, N:2 * N]
    assert vd.stride(0) != tkv * vd.stride(1) and vd.stride(1) != N and vd.data_ptr() % 16 == 0
    return t(k), vd


def to_q(C, a, w, scale, bias0):
    """The first launch of the chain: mixdq_qlinear_w8a8 to fp16."""
    return C.qlinear_w8_a8_ohalf(a, w, scale, scal(1), scal(0), bias0, scale, bias0, None)


@pytest.mark.parametrize("tkv", ei.QATT_KEY_COUNTS)
def test_selection_returns_the_hot_value_row_bit_for_bit(C, oracle, tkv):
    s, z = scal(S_INV), scal(ZP)
    for tq in ei.QATT_QUERY_COUNTS:
        o = ei.toq_operands("selection", tkv, tq)
        c = o["case"]
        want = c["expected"]
        want8 = oracle.quantize(want, S_INV, ZP, C.FLAGS & 1)
        assert (want8 != want8.flat[0]).any()
        a, scale, bias0 = t(o["a"]), t(o["scale"]), t(o["bias0"])
        for wbits in WBITS:
            w, kw = stored(o["w"], wbits)
            for layout in KV_LAYOUTS:
                k, v = kv_views(c["k"], c["v"], layout, tkv)
                what = f"selection k{tkv} q{tq} W{wbits} {layout}"
                got = C.qlinear_attention(a, w, scale, bias0, k, v, **kw)
                assert got.shape == want.shape and got.dtype == torch.float16
                assert_bits(got, want, what, c)
                o8 = C.qlinear_attention(a, w, scale, bias0, k, v, s, z, **kw)
                assert o8.dtype == torch.int8 and np.array_equal(o8.cpu().numpy(), want8), what + " INT8"
                o4 = C.qlinear_attention(a, w, scale, bias0, k, v, s, z, _abits=4, **kw)
                assert np.array_equal(o4.cpu().numpy(), np.minimum(want8, -113)), what + " A4"


@pytest.mark.parametrize("tkv", ei.QATT_KEY_COUNTS)
def test_every_key_is_counted_exactly_once(C, tkv):
    for tq in ei.QATT_QUERY_COUNTS:
        o = ei.toq_operands("every_key_once", tkv, tq)
        c = o["case"]
        a, scale, bias0 = t(o["a"]), t(o["scale"]), t(o["bias0"])
        ints = ei.toq_operands("small_integers", tkv, tq) if c["exact"] else None
        for wbits in WBITS:
            w, kw = stored(o["w"], wbits)
            for layout in KV_LAYOUTS:
                k, v = kv_views(c["k"], c["v"], layout, tkv)
                what = f"probes k{tkv} q{tq} W{wbits} {layout}"
                got = C.qlinear_attention(a, w, scale, bias0, k, v, **kw)
                g = got.cpu().numpy().astype(np.float64)
                bad = np.argwhere(np.abs(g - c["expected"]) > c["ulp"])
                if len(bad):
                    b, i, ch = (int(x) for x in bad[0])
                    keys = sorted({int(c["probes"][int(bb), int(cc)]) for bb, _, cc in bad})
                    raise AssertionError(f"{what}: {len(bad)} outputs off; first batch {b} query {i} channel {ch}: got "
                                         f"{g[b, i, ch]!r} want {c['expected'][b, i, ch]!r}; probe keys involved {keys[:16]}")
                if c["exact"]:
                    assert_bits(got, c["expected16"], what)
                    si = ints["case"]
                    wi, _ = stored(ints["w"], wbits)
                    ki, vi = kv_views(si["k"], si["v"], layout, tkv)
                    assert_bits(C.qlinear_attention(t(ints["a"]), wi, scale, bias0, ki, vi, **kw), si["expected"],
                                f"integer mean k{tkv} q{tq} W{wbits} {layout}")


def test_small_integer_key_counts():
    assert [n for n in ei.QATT_KEY_COUNTS if n & (n - 1) == 0] == [1, 4, 64, 128]


RESCALE = [(kind, tkv) for kind in ei.RESCALE_KINDS for tkv in ei.QATT_RESCALE_KEY_COUNTS]


def huge_values_operands(tkv, tq):
    """Random int8 operands whose to_q output is N(0, ~1.2^2), with the k / v of rescale("huge_values")."""
    c = ei.rescale("huge_values", 64, tkv, tq, ei.QATT_B, HEADS)
    N, K = HEADS * 64, 256
    a, w = dd.int8(7000 + tkv, (ei.QATT_B, tq, K)), dd.int8(7001 + tkv, (N, K))
    sd = K ** 0.5 * np.std(a.astype(np.float64)) * np.std(w.astype(np.float64))
    return dict(a=a, w=w, scale=np.full(N, 1.2 / sd, np.float32), bias0=np.zeros(N, np.float32), q=None, case=c)


@pytest.mark.parametrize("kind,tkv", RESCALE, ids=[f"{k}_k{n}" for k, n in RESCALE])
def test_rescale_path_and_extremes(C, oracle, kind, tkv):
    tq = 64
    o = huge_values_operands(tkv, tq) if kind == "huge_values" else ei.toq_operands("rescale", tkv, tq, kind)
    c = o["case"]
    B = o["a"].shape[0]
    a, w, scale, bias0 = t(o["a"]), t(o["w"]), t(o["scale"]), t(o["bias0"])
    k, v = kv_views(c["k"], c["v"], "packed")
    q16 = to_q(C, a, w, scale, bias0)
    if o["q"] is not None:
        assert_bits(q16, o["q"], f"to_q {kind} k{tkv}")                 # the prescribed Q: the builder's expected holds
    q_host = q16.cpu().numpy()
    _, ref64 = oracle.attention_f16(q_host, c["k"], c["v"], HEADS)
    if o["q"] is not None:
        assert np.abs(ref64 - c["expected"]).max() <= 1e-12 * np.abs(c["v"].astype(np.float64)).max()
    got = C.qlinear_attention(a, w, scale, bias0, k, v)
    chain = C.attention_f16(q16, k, v, HEADS)
    g, g2 = (x.cpu().numpy().astype(np.float64) for x in (got, chain))
    tol = ATOL + RTOL * np.abs(ref64)
    err, err2 = np.abs(g - ref64), np.abs(g2 - ref64)
    with np.errstate(invalid="ignore"):
        print(f"{kind} k{tkv}: fused max err {err.max():.3e} (worst err / tol {np.nanmax(err / tol):.3f}); attention_f16 on "
              f"the same Q max err {np.nanmax(err2):.3e} (worst err / tol {np.nanmax(err2 / tol):.3f}); "
              f"max |ref| {np.abs(ref64).max():.4g}")
    assert np.isfinite(g).all()
    assert (err <= tol).all(), f"max err {err.max():.3e}, worst err / tol {(err / tol).max():.3f}"
    # a convex combination: every channel within the range of its head's values, up to one ulp of the bound
    v64 = c["v"].astype(np.float64)
    lo, hi = v64.min(axis=1, keepdims=True), v64.max(axis=1, keepdims=True)
    assert (g >= lo - ei.ulp16(lo)).all() and (g <= hi + ei.ulp16(hi)).all()
    for cfg in (0, 1):               # the library's choice and the short-key kernel
        assert torch.equal(C.attention_f16(q16, k, v, HEADS, _cfg=cfg).view(torch.int16), got.view(torch.int16)), \
            f"attention_f16(to_q) form {cfg}"
    for b in range(B):
        one = C.qlinear_attention(a[b:b + 1], w, scale, bias0, k[b:b + 1], v[b:b + 1])
        assert torch.equal(one[0].view(torch.int16), got[b].view(torch.int16)), f"image {b} alone"


def _g(name, B=1, T=64, N=256, K=256, tkv=77, layout="packed", softmax_scale=None):
    return dict(name=name, B=B, T=T, N=N, K=K, tkv=tkv, layout=layout, softmax_scale=softmax_scale)


GEOMETRY = (
    [_g(f"ktiles{K // 128}", B=2, K=K) for K in (128, 256, 384, 512, 1024)]              # against three stages
    + [_g("five_images_of_one_tile", B=5, N=128)]                                        # img = m0 / att_tq per M tile
    + [_g("one_n_tile", T=128, N=128, tkv=97, layout="contiguous"), _g("three_n_tiles", T=128, N=384, tkv=97, layout="mixed")]
    + [_g(f"scale{s:.4g}_k{n}", tkv=n, softmax_scale=s) for s in (0.2, 1 / 16) for n in (77, 128)]
    + [_g(f"keys{n}", tkv=n, layout="mixed") for n in (1, 2, 3, 4, 5, 8, 60, 61, 67, 68, 124, 125)])


@pytest.mark.parametrize("case", GEOMETRY, ids=[c["name"] for c in GEOMETRY])
def test_geometry_equals_the_two_launch_chain(C, oracle, case):
    B, T, N, K, tkv, ss = (case[n] for n in ("B", "T", "N", "K", "tkv", "softmax_scale"))
    seed = 8000 + 7 * K + N + tkv
    a, w = t(dd.int8(seed, (B, T, K))), t(dd.int8(seed + 1, (N, K)))
    scale = t(dd.f32(seed + 2, (N,), 1e-5, 6e-5) * np.float32((256 / K) ** 0.5))       # q of a few units at every K
    bias0 = t(dd.f32(seed + 3, (N,), -300, 300))
    kh, vh = dd.normal_f16(seed + 4, (B, tkv, N), 1.0), dd.normal_f16(seed + 5, (B, tkv, N), 1.0)
    k, v = kv_views(kh, vh, case["layout"], seed)
    s_inv, zp = scal(30.0), scal(-3.0)
    q16 = to_q(C, a, w, scale, bias0)
    want = C.attention_f16(q16, k, v, N // 64, softmax_scale=ss)
    got = C.qlinear_attention(a, w, scale, bias0, k, v, softmax_scale=ss)
    assert got.dtype == torch.float16 and tuple(got.shape) == (B, T, N)
    assert_bits(got, want.cpu().numpy(), case["name"])
    want8 = C.attention_f16(q16, k, v, N // 64, s_inv, zp, softmax_scale=ss)
    got8 = C.qlinear_attention(a, w, scale, bias0, k, v, s_inv, zp, softmax_scale=ss)
    assert got8.dtype == torch.int8 and torch.equal(got8, want8), case["name"] + " INT8"
    _, ref = oracle.attention_f16(q16.cpu().numpy(), kh, vh, N // 64, ss)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    assert (err <= ATOL + RTOL * np.abs(ref)).all(), f"max err {err.max():.3e}"
    if ss is not None:               # the scale reaches the kernel: the default's result is another one
        assert not torch.equal(got, C.qlinear_attention(a, w, scale, bias0, k, v))


def _raw_call(C, b, M, N, K, T, tkv, k_rs, v_rs, sinv=None, zp=None):
    code = C._lib.mixdq_qlinear_w8a8_attn(_p(b["A"]), _p(b["W"]), _p(b["bias0"]), _p(b["scale"]), _p(b["k"]), _p(b["v"]),
                                          _p(b["D"]), M, N, K, T, tkv, tkv * k_rs, k_rs, tkv * v_rs, v_rs, 0.125,
                                          sinv, zp, C.FLAGS, _stream())
    return _sync_status(code)


def test_refusals_stay_refusals(C):
    """The status from the C entry with an output full of sentinel bytes between guards, and the wrapper's error.  Every
    buffer is as large as the nearest accepted shape needs, whatever the call claims."""
    B, T, N, K, tkv = 1, 128, 256, 256, 77
    rows = 2 * 64                                                   # key rows allocated: two whole tiles
    arrs = dict(A=dd.int8(8800, (B * T, K)), W=dd.int8(8801, (N, K)), bias0=dd.f32(8802, (N,), -30, 30),
                scale=dd.f32(8803, (N,), 1e-4, 6e-4), k=dd.normal_f16(8804, (rows + 2, N + 8), 1.0),
                v=dd.normal_f16(8805, (rows + 2, N + 8), 1.0), D=np.zeros((B * T, N), np.float16))
    one = scal(20.0)
    ptr = ctypes.c_void_p(one.data_ptr())
    refused = [  # what, (M, N, K, T, tkv, k_rs, v_rs), quantizer pointers, status
        ("tkv = 129", (128, N, K, 128, 129, N, N), (None, None), ERR_SHAPE),
        ("T % 64", (100, N, K, 100, tkv, N, N), (None, None), ERR_SHAPE),
        ("N % 128", (128, 192, K, 128, tkv, 192, 192), (None, None), ERR_SHAPE),
        ("K % 128", (128, N, 192, 128, tkv, N, N), (None, None), ERR_SHAPE),
        ("k row stride % 8", (128, N, K, 128, tkv, N + 4, N), (None, None), ERR_ALIGNMENT),
        ("scale_inv alone", (128, N, K, 128, tkv, N, N), (ptr, None), ERR_INVALID_ARG),
        ("zero_point alone", (128, N, K, 128, tkv, N, N), (None, ptr), ERR_INVALID_ARG),
    ]
    for what, shape, (sinv, zp), status in refused:
        b = {n: Buf(x, sentinel=n == "D") for n, x in arrs.items()}
        assert _raw_call(C, b, *shape, sinv, zp) == status, what
        assert b["D"].still_sentinel(), what + ": the refused launch wrote"
    b = {n: Buf(x, sentinel=n == "D") for n, x in arrs.items()}     # ... and the accepted call writes every element
    assert _raw_call(C, b, 128, N, K, 128, tkv, N + 8, N + 8) == 0 and b["D"].untouched() and not b["D"].still_sentinel()
    kd, vd = (t(arrs[n])[None, :tkv, :N] for n in "kv")              # the same strided rows through the wrapper
    assert_bits(C.qlinear_attention(t(arrs["A"])[None], t(arrs["W"]), t(arrs["scale"]), t(arrs["bias0"]), kd, vd),
                b["D"].value()[None], "C entry vs wrapper")
    # the wrapper
    a, w, sc, b0 = t(arrs["A"].reshape(B, T, K)), t(arrs["W"]), t(arrs["scale"]), t(arrs["bias0"])
    k = t(dd.normal_f16(8806, (B, tkv, N), 1.0))
    assert C.qlinear_attention(a, w, sc, b0, k, k).shape == (B, T, N)
    k129 = t(dd.normal_f16(8807, (B, 129, N), 1.0))
    k192 = t(dd.normal_f16(8808, (B, tkv, 192), 1.0))
    for what, args in (("tkv = 129", (a, w, sc, b0, k129, k129)), ("T % 64", (a[:, :100], w, sc, b0, k, k)),
                       ("N % 128", (a, w[:192], sc[:192], b0[:192], k192, k192)),
                       ("K % 128", (a[..., :192].contiguous(), w[:, :192].contiguous(), sc, b0, k, k))):
        assert not C.qlinear_attention_supported(args[0].shape, args[1].shape[0], args[1].shape[1], args[4]), what
        with pytest.raises(RuntimeError, match="unsupported configuration"):
            C.qlinear_attention(*args)
    odd = t(dd.normal_f16(8809, (B, tkv, N + 4), 1.0))[..., :N]     # row stride 260 elements
    assert odd.stride(1) % 8 == 4 and odd.data_ptr() % 16 == 0
    with pytest.raises(RuntimeError, match="qlinear_attention"):
        C.qlinear_attention(a, w, sc, b0, odd, k)
