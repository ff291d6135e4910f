"""CPU checks of tests/heavy_acc.py: its operands reach the regime they are built for (accumulators FP32 cannot
hold, exact ties, both signs, a control), the oracle and its numpy mirror equal the integer expectation bit for bit
in both epilogue variants, and a conversion that truncates, or rounds halves away, is rejected on every case.
No tolerance anywhere: integers computed without floats, or the oracle's bits."""
import numpy as np
import pytest

from tests import heavy_acc as ha
from tests import tile_edges as te

LINEAR = ha.host_linear_cases()
CONV = ha.all_conv_cases()


def lin_id(c):
    return f"m{c[0]}_n{c[1]}_k{c[2]}_q{-c[3]}{'_geglu' if c[4] else ''}"


def conv_id(c):
    return f"n{c[0]}_{c[1]}x{c[2]}_c{c[3]}_k{c[4]}_q{-c[5]}{'_ups' if len(c) > 6 and c[6] else ''}"


def shares(c, what, reach):
    """The per-case conditions on the inputs; prints the shares (DESIGN.md section 4 quotes them)."""
    acc = c.acc
    cls = np.broadcast_to(c.cls, acc.shape)
    big = np.abs(acc) >= 1 << 24
    ix, ti = ha.inexact(acc), ha.tie(acc)
    pos, neg = (acc[big] > 0).mean(), (acc[big] < 0).mean()
    ctl = (cls == 5) & ~ix
    rtz = (ha.round_f32(acc, "rtz") != ha.round_f32(acc)).mean()
    rha = (ha.round_f32(acc, "rha") != ha.round_f32(acc)).mean()
    print(f"{what}: inexact {ix.mean():.3f} ties {ti.mean():.3f} positive {pos:.3f} negative {neg:.3f} "
          f"control {ctl.mean():.3f} truncation differs {rtz:.3f} half-away differs {rha:.3f} "
          f"max |acc| {int(np.abs(acc).max())}")
    assert ix.mean() >= 0.20 and ti.mean() >= 0.10 and ctl.mean() >= 0.10
    assert pos >= 0.10
    if ha.negative_reachable(reach, c.qmin):
        assert neg >= 0.10
    assert not ix[cls == 5].any(), "a control accumulator is inexact"
    assert rtz > 0 and rha > 0
    return rtz, rha


def test_integer_rounding_is_the_fp32_conversion():
    """round_f32 against numpy's int -> float32 conversion (RNE) on values around every spacing change, and the FP16
    assembly against numpy's bits: the two float casts of this file, of the helpers, not of an expectation."""
    rng = np.random.default_rng(3)
    v = np.concatenate([(1 << k) + rng.integers(-300, 300, 4000) for k in range(22, 31)] +
                       [rng.integers(-(1 << 31) + 1, 1 << 31, 100000)])
    v = np.concatenate([v, -v])
    assert np.array_equal(ha.round_f32(v), v.astype(np.float32).astype(np.int64))
    assert (ha.round_f32(v, "rtz") != ha.round_f32(v)).any() and (ha.round_f32(v, "rha") != ha.round_f32(v)).any()
    assert np.array_equal(np.abs(ha.round_f32(v, "rtz")) <= np.abs(v), np.ones(v.size, bool))
    i = np.concatenate([np.arange(-2048, 2049), 2 * np.arange(-2048, 2049), 128 * np.arange(-60, 61)])
    assert np.array_equal(ha.f16_bits(i), i.astype(np.float16).view(np.uint16))
    with pytest.raises(AssertionError):
        ha.f16_bits(np.asarray([2049]))


def test_class_counts_are_the_stated_ones():
    free = ha.K_INT8 - ha.K_INT8 // 64
    assert [ha._k0(c, free, -128)[0] for c in range(5)] == [1025, 1033, 2049, 2065, 4097]
    assert ha._k0(6, free, -128) == (1024, -128) and ha._k0(7, free, -128) == (free, -128)
    assert [ha._conv_count(c, 256, 252, -128)[0] for c in range(8)] == [114, 115, 228, 230, 171, 0, 256, 252]
    c = ha.linear(17, 72, ha.K_INT8)
    assert int(c.base[0, 6]) == 1 << 24                                   # class 6: exactly 2^24
    for n in range(8):                                                    # the rail weights lie in every K-tile
        rail = (c.w[n] == (127 if n in (1, 3) else -128)).reshape(-1, 128).sum(axis=1)
        assert (rail > 0).all() or n == 5
    cv = ha.conv(*ha.CONV_SHAPE, ha.CONV_C, 72)
    assert int(cv.base[0, 0, 0, 6]) == 1 << 24 and int(cv.base[1, 15, 15, 6]) == 1 << 24      # corners, all -128
    assert int(cv.acc.max()) > 37_000_000 and 24_000_000 < int(cv.acc[0, 0, 5, 7]) < 26_000_000


@pytest.mark.parametrize("case", LINEAR, ids=[lin_id(c) for c in LINEAR])
def test_linear_operands_and_references(oracle, case):
    M, N, K, qmin, geglu = case
    c = ha.linear(*case)
    assert int(np.abs(c.delta).max()) <= (127 if geglu else 2047)
    shares(c, lin_id(case), K)
    D = N // 2 if geglu else N
    for variant in (0, 1):
        out, acc = oracle.qlinear(c.a, c.w, c.bias0, c.scale, getattr(c, "bias", None), variant, return_acc=True)
        assert np.array_equal(acc[:, :D].astype(np.int64), c.acc), "the gathered delta is not the accumulator's"
        assert np.array_equal(out.view(np.uint16)[:, :D], c.want), f"oracle != integer expectation, variant {variant}"
        mirror = oracle.np_qlinear(c.a, c.w, c.bias0, c.scale, getattr(c, "bias", None), variant)
        assert np.array_equal(mirror.view(np.uint16), out.view(np.uint16)), f"numpy mirror, variant {variant}"
        if geglu:
            assert (out[:, D:] == np.float16(16)).all()
            q, _ = oracle.geglu_quantize(out, 1.0 / 16, 0.0, variant)       # gelu(16) == 16 in the specification
            assert np.array_equal(q, c.want_q), "value * gelu(16) / 16 is not the value"
    for mode in ("rtz", "rha"):                                             # a wrong reference is rejected
        assert (ha.wrong(c, mode) != c.want_int).any(), mode
        if not geglu:
            acc32 = c.acc.astype(np.int64)
            bad = oracle.np_epilogue(ha.round_f32(acc32, mode), c.bias0[None, :], c.scale[None, :])
            assert not np.array_equal(bad.view(np.uint16), c.want), mode


@pytest.mark.parametrize("case", [c for c in LINEAR if not c[4]], ids=[lin_id(c) for c in LINEAR if not c[4]])
def test_linear_fp16_end(oracle, case):
    c = ha.linear(*case)
    scale, bias, residual, sclass = ha.fp16_end(c)
    for variant in (0, 1):
        out = oracle.qlinear(c.a, c.w, c.bias0, scale, bias, variant)
        assert np.array_equal(oracle.np_qlinear(c.a, c.w, c.bias0, scale, bias, variant).view(np.uint16),
                              out.view(np.uint16)), f"numpy mirror, variant {variant}"
        assert not np.isnan(out).any() and not np.isnan(oracle.add_f16(out, residual)).any()
        f = out.astype(np.float64)
        assert sorted(set(sclass)) == [0, 1, 2, 3]
        one = np.abs(f[:, sclass == 0])
        assert ((one > 2.0 ** -3) & (one < 4)).any()
        assert (np.abs(f[:, sclass == 1] - bias[sclass == 1].astype(np.float64)) < 2.0 ** -9).all()   # 2^-20 * delta + bias
        over = f[:, sclass == 2]
        assert np.isinf(over).any() and (np.isfinite(over) & (np.abs(over) > 32768)).any()
        sub = np.abs(f[:, sclass == 3])
        assert ((sub > 0) & (sub < 2.0 ** -14)).any() and (sub < 2.0 ** -13).all()
    # a wrong conversion shows here too
    for mode in ("rtz", "rha"):
        bad = oracle.np_epilogue(ha.round_f32(c.acc, mode), c.bias0[None, :], scale[None, :], bias[None, :])
        assert not np.array_equal(bad.view(np.uint16), out.view(np.uint16)), mode


@pytest.mark.parametrize("case", CONV, ids=[conv_id(c) for c in CONV])
def test_conv_operands_and_references(oracle, case):
    c = ha.conv(*case)
    shares(c, conv_id(case), 9 * c.C)
    for variant in (0, 1):
        out, acc = oracle.qconv2d(c.x, c.w, c.scale, c.wsum, float(ha.ZP), None, None, 1, 1, variant, return_acc=True)
        assert np.array_equal(acc.astype(np.int64), c.acc), "window intersection is not the accumulator's"
        assert np.array_equal(out.view(np.uint16), c.want), f"oracle != integer expectation, variant {variant}"
    for mode in ("rtz", "rha"):
        assert (ha.round_f32(c.acc, mode) - c.base != c.want_int).any(), mode
    if case[5] == -128 and case[3] == ha.CONV_C:                            # the FP16 end
        scale, bias, residual, sclass = ha.fp16_end(c)
        out = oracle.qconv2d(c.x, c.w, scale, c.wsum, float(ha.ZP), None, bias, 1, 1, 0)
        assert not np.isnan(out).any() and np.isinf(out).any()
        b0 = -c.base.astype(np.float32)                                     # (multiples of 128: exact)
        mirror = oracle.np_epilogue(c.acc.astype(np.int32), -b0, scale, bias, 0)
        assert np.array_equal(mirror.view(np.uint16), out.view(np.uint16))


def test_cases_follow_the_tables():
    """Every INT8 tile id, every GEGLU-admissible one, every halo tile and every LN tile has its problem."""
    lin = set(LINEAR)
    for cfg in te.IGEMM:
        assert all(shape + (-128, False) in lin for shape in ha.gemm_shapes(cfg))
        assert ha.CONV_SHAPE + (ha.CONV_C, ha.conv_k(te.tile(cfg)[1]), -128) in set(CONV)
        if te.geglu_admissible(cfg):
            assert ha.geglu_shape(cfg) + (-128, True) in lin
    assert set(ha.LN_TILES) <= set(te.AQ) and len(ha.HALO) >= 4
    for bits in (4, 2):
        assert len(ha.packed_tiles(bits)) == 2
