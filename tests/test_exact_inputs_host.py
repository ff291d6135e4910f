"""The exact-result inputs of tests/exact_inputs.py, checked on the CPU (no GPU): every builder case the GPU files
run is built here (each builder asserts its own precondition in float64), its stated expected output is compared
with the float64 oracle / an int64 evaluation, and the cases are shown to reach every edge they are meant to reach
-- the edges are restated here, independently of the generator."""
import numpy as np
import pytest

from tests import exact_inputs as ei
from tests import tile_edges as te

CASES = [(D, tkv) for D in ei.WIDTHS for tkv in ei.KEY_COUNTS]
IDS = [f"d{D}_k{tkv}" for D, tkv in CASES]


def required_keys(tkv):
    """First, last, both sides of every 64-key tile boundary, both sides of the last 4-key group boundaries (the
    mask limit tkv - 64 t - 4 hh moves in fours between the half-waves)."""
    need = {0, tkv - 1}
    for t in range(1, (tkv + 63) // 64):
        need |= {64 * t - 1, 64 * t}
    g = 4 * ((tkv - 1) // 4)                       # first key of the last (possibly partial) group of four
    need |= {k for k in (g - 5, g - 4, g - 1, g) if k >= 0}
    return need


def test_the_case_list_covers_the_stated_key_and_query_counts():
    assert {1, 63, 64, 65, 77, 127, 128, 129, 130, 256, 300, 640, 1024, 4096, 4097} <= set(ei.KEY_COUNTS)
    assert {1, 4, 5, 32, 33, 63} <= {n % 64 for n in ei.KEY_COUNTS}
    assert set(ei.WIDTHS) == {64, 40, 80, 160}
    tqs = {ei.query_count(n) for n in ei.KEY_COUNTS}
    assert all(tq % 64 and tq % 128 for tq in tqs)                     # ragged against both workgroup shapes
    assert any(ei.query_count(n) == n for n in ei.KEY_COUNTS)          # the fused q|k|v layout occurs
    assert any(n <= 128 for n in ei.KEY_COUNTS) and any(n > 64 * 4 for n in ei.KEY_COUNTS)   # short form; ring wrap
    assert {p for p in ei.KEY_COUNTS if p & (p - 1) == 0} >= {1, 64, 128, 256, 1024, 4096}


@pytest.mark.parametrize("D,tkv", CASES, ids=IDS)
def test_selection_cases(oracle, D, tkv):
    c = ei.selection(D, tkv)
    q, k, v, heads, hot, want = c["q"], c["k"], c["v"], c["heads"], c["hot"], c["expected"]
    B, tq, Cc = q.shape
    assert tq == ei.query_count(tkv) and k.shape == v.shape == (B, tkv, Cc)
    assert set(np.abs(k.astype(np.float64)).ravel()) == {ei.AMPLITUDE[D]}           # sign codes
    # the stated precondition, restated: gap >= 26 log2 units, hot score <= 1000
    st = c["stats"]
    assert st["min_gap"] >= 26 and 0 < st["min_hot"] <= st["max_hot"] <= 1000 and st["max_rest_ulps"] <= 1 / 16
    # the oracle: its FP16 result IS the hot value row, its float64 result within 1/8 ulp of it
    ref16, ref64 = oracle.attention_f16(q, k, v, heads)
    assert np.array_equal(ref16.view(np.uint16), want.view(np.uint16))
    assert (np.abs(ref64 - want.astype(np.float64)) <= ei.ulp16(want) / 8).all()
    for b in range(B):
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            assert np.array_equal(want[b, :, sl].view(np.uint16), v[b, hot[b, h], sl].view(np.uint16))
            reached = set(int(x) for x in hot[b, h])
            assert reached == set(range(tkv)) if tq >= tkv else required_keys(tkv) <= reached, (b, h)
    vals = {cls: np.abs(np.concatenate([v[b, :, h * D:(h + 1) * D].ravel() for (b, h), x in c["classes"].items()
                                        if x == cls]).astype(np.float64)) for cls in ei.CLASSES}
    assert vals["huge"].max() >= 6e4 or tkv < 4
    assert ((vals["subnormal"] > 0) & (vals["subnormal"] < 2.0 ** -14)).any()
    assert 1 / 32 <= vals["unit"].min() and vals["unit"].max() <= 2
    assert (v != 0).all()                                                            # (the sign of a zero is not pinned)


def test_selection_refuses_inputs_that_miss_its_precondition(monkeypatch):
    monkeypatch.setitem(ei.AMPLITUDE, 64, 1.0)                # gaps of 2 h log2(e) / 8 per differing sign: too small
    with pytest.raises(AssertionError, match="gap"):
        ei.selection.__wrapped__(64, 300)
    monkeypatch.setitem(ei.AMPLITUDE, 64, 12.0)               # hot score 144 * 8 * log2(e) > 1000
    with pytest.raises(AssertionError, match="hot score"):
        ei.selection.__wrapped__(64, 300)
    with pytest.raises(AssertionError):
        ei.small_integers.__wrapped__(64, 300)                # not a power of two
    with pytest.raises(AssertionError):
        ei.small_integers.__wrapped__(64, 4096, vmax=4096)    # tkv * max|v| >= 2^24 (and not FP16 integers)
    with pytest.raises(AssertionError):
        ei.f16_epilogue(np.array([2 ** 20]), None, None)


@pytest.mark.parametrize("D,tkv", CASES, ids=IDS)
def test_every_key_once_cases(oracle, D, tkv):
    c = ei.every_key_once(D, tkv)
    _, ref64 = oracle.attention_f16(c["q"], c["k"], c["v"], c["heads"])
    assert np.abs(ref64 - c["expected"]).max() <= 1e-12 * ei.PROBE / tkv
    assert (c["expected"] == 2048.0 / tkv).all() and c["exact"] == (tkv & (tkv - 1) == 0)
    v = c["v"].astype(np.float64)
    assert ((v != 0).sum(axis=1) == 1).all() and set(np.unique(v)) <= {0.0, 2048.0}   # one probe per channel
    B, _, Cc = v.shape
    assert Cc == c["heads"] * D
    assert required_keys(tkv) | {tkv - 1} <= set(int(x) for x in c["probes"].ravel())
    for b in range(B):
        assert (v[b, c["probes"][b], np.arange(Cc)] == 2048.0).all()
    if c["exact"]:
        s = ei.small_integers(D, tkv)
        _, ref64 = oracle.attention_f16(s["q"], s["k"], s["v"], s["heads"])
        vi = s["v"].astype(np.int64)
        assert np.array_equal(vi.astype(np.float16), s["v"]) and tkv * np.abs(vi).max() < 2 ** 24
        assert np.abs(ref64 - s["mean"][:, None, :]).max() <= 1e-12 * max(1.0, np.abs(s["mean"]).max())
        assert np.array_equal(s["expected"][:, 0], (vi.sum(axis=1) / tkv).astype(np.float16))
        assert np.abs(vi).max() >= 32 and len(np.unique(s["expected"])) > 16


RESCALE = [(kind, D, tkv) for kind in ei.RESCALE_KINDS for D in ei.WIDTHS for tkv in ei.RESCALE_KEY_COUNTS]


@pytest.mark.parametrize("kind,D,tkv", RESCALE, ids=[f"{k}_d{D}_k{n}" for k, D, n in RESCALE])
def test_rescale_cases(oracle, kind, D, tkv):
    c = ei.rescale(kind, D, tkv)
    _, ref64 = oracle.attention_f16(c["q"], c["k"], c["v"], c["heads"])
    scale = np.abs(c["v"].astype(np.float64)).max()
    assert np.abs(ref64 - c["expected"]).max() <= 1e-12 * scale
    tm = c["facts"]["tile_max"]                                  # [B, heads, tq, tiles], log2 units
    d = np.median(np.diff(tm, axis=-1), axis=(0, 1, 2))          # per tile boundary, the typical query
    if kind in ("rise4", "rise40", "fall4", "fall40"):
        step = (40.0 if kind.endswith("40") else 4.0) * (1 if kind.startswith("rise") else -1)
        assert len(d) >= 1 and (np.abs(d - step) <= 0.25 * abs(step)).all(), d       # alpha = 2^-|step| per tile
    elif kind == "late_dominant":
        first, last, mid = np.median(tm[..., 0]), np.median(tm[..., -1]), np.median(tm[..., 1:-1]) if tm.shape[-1] > 2 else 0
        assert first >= 40 and last >= first + 40 and mid <= 10
    elif kind.startswith("equal_large"):
        sign = -1 if kind.endswith("negative") else 1
        assert np.abs(c["scores"] - 60.0 * sign).max() <= 0.5
    else:
        assert 5.9e4 <= scale <= 65504 and np.abs(c["v"].astype(np.float64)).min() >= 2.9e4
        assert (np.sign(c["v"]) == np.sign(c["v"][:, :1])).all()                         # one sign per channel


def test_rescale_key_counts_reach_the_short_form_the_ragged_mask_and_the_ring_wrap():
    assert any(n <= 128 and n % 64 for n in ei.RESCALE_KEY_COUNTS)
    assert any(n > 128 and n % 64 for n in ei.RESCALE_KEY_COUNTS)
    assert any(n % 64 == 0 and n // 64 > 4 for n in ei.RESCALE_KEY_COUNTS)
    assert ei.rescale("rise4", 64, 300)["q"].shape[0] >= 2                              # a batch: rows vs single runs


# ------------------------------------------------------------------------------------------ FP16 layers
def check_values(c, x="x", w="w"):
    xv, wv = c[x].astype(np.float64), c[w].astype(np.float64)
    assert np.array_equal(xv, np.round(xv)) and np.abs(xv).max() <= 4 and np.array_equal(wv, np.round(wv)) \
        and np.abs(wv).max() <= 2
    for name in ("bias", "residual"):
        if c.get(name) is not None:
            b = c[name].astype(np.float64) * 8
            assert np.array_equal(b, np.round(b)) and np.abs(b).max() <= 32


def int64_linear(c, rows=None):
    x = c["x"].astype(np.int64) if rows is None else c["x"][rows].astype(np.int64)
    acc = x @ c["w"].astype(np.int64).T
    res = None if c["residual"] is None else (c["residual"] if rows is None else c["residual"][rows])
    return ei.f16_epilogue(acc, c["bias"], res)


F16L = te.all_f16()


@pytest.mark.parametrize("case", F16L, ids=[te.f16_id(c) for c in F16L])
def test_linear_tile_edge_expectations_equal_an_int64_evaluation(case):
    c = ei.linear(case["M"], case["K"], case["N"], case["bias"], True)
    check_values(c)
    assert np.array_equal(int64_linear(c).view(np.uint16), c["expected"].view(np.uint16))


@pytest.mark.parametrize("M,K,N,bias", ei.LIN)
def test_linear_layer_expectations_equal_an_int64_evaluation(M, K, N, bias):
    c = ei.linear(M, K, N, bias, False)
    check_values(c)
    rows = None if M * K * N <= 1 << 27 else np.unique(np.r_[0, M - 1, (np.arange(40) * 7919) % M])   # int64 matmul is slow
    want = c["expected"] if rows is None else c["expected"][rows]
    assert np.array_equal(int64_linear(c, rows).view(np.uint16), want.view(np.uint16))


def test_linear_cases_reach_long_k_and_a_rounding_that_matters():
    assert max(k for _, k, _, _ in ei.LIN) == 5120 and any(k % 64 for _, k, _, _ in ei.LIN)
    c = ei.linear(1024, 5120, 1280, True, False)
    exact = c["x"][:64].astype(np.float64) @ c["w"].astype(np.float64).T + c["bias"].astype(np.float64)
    got = c["expected"][:64].astype(np.float64)
    inexact = got != exact
    assert inexact.mean() > 0.1 and np.abs(exact).max() < 2 ** 20            # fp16(acc + bias) really rounds
    tie = np.abs(np.abs(got - exact) - ei.ulp16(exact) / 2) == 0
    assert tie.any()                                                       # ... ties to even included
    assert (np.abs(got - exact) <= ei.ulp16(exact) / 2).all()


@pytest.mark.parametrize("case", ei.CONV, ids=[f"c{c[1]}_k{c[4]}_{c[5]}x{c[5]}_s{c[6]}p{c[7]}" for c in ei.CONV])
def test_conv_expectations_equal_an_int64_evaluation(case):
    for residual in (None, "full", "per_image"):
        c = ei.conv2d(*case, residual=residual)
        check_values(c)
        acc = ei.conv_accumulate(c["x"].astype(np.int64), c["w"].astype(np.int64), case[6], case[7], np.int64)
        res = c["residual"] if residual != "per_image" else c["residual"][:, :, None, None]
        want = ei.f16_epilogue(acc, None if c["bias"] is None else c["bias"][None, :, None, None], res)
        assert np.array_equal(want.view(np.uint16), c["expected"].view(np.uint16))
        # an independent evaluation of one output element per case: the plain triple loop of the definition
        n, k, p, q = acc.shape[0] - 1, acc.shape[1] - 1, acc.shape[2] // 2, acc.shape[3] - 1
        s = 0
        for r in range(case[5]):
            for t in range(case[5]):
                y, xx = p * case[6] + r - case[7], q * case[6] + t - case[7]
                if 0 <= y < case[2] and 0 <= xx < case[3]:
                    s += int((c["x"][n, :, y, xx].astype(np.int64) * c["w"][k, :, r, t].astype(np.int64)).sum())
        assert s == acc[n, k, p, q]


def test_conv_cases_reach_the_stated_forms():
    assert any(c[1] == 4 for c in ei.CONV) and any(c[4] == 4 for c in ei.CONV)       # generic C = 4 kernel; K = 4
    assert any(c[6] == 2 for c in ei.CONV) and {0, 1} <= {c[7] for c in ei.CONV}
    assert {1, 3} <= {c[5] for c in ei.CONV} and {True, False} == {c[8] for c in ei.CONV}


@pytest.mark.parametrize("M,K,N", ei.GEMM)
def test_gemm_expectations_equal_an_int64_evaluation(M, K, N):
    c = ei.gemm(M, K, N)
    check_values(c, "a", "b")
    want = ei.f16_epilogue(c["a"].astype(np.int64) @ c["b"].astype(np.int64), None, None)
    assert np.array_equal(want.view(np.uint16), c["expected"].view(np.uint16))


# ------------------------------------------------------------------------------------------ norm producers
def test_fma32_is_the_correctly_rounded_fma():
    from fractions import Fraction
    a = dd_f32(1, 4000)
    b = dd_f32(2, 4000)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + dd_f32(3, 4000).astype(np.float64) * 1e-6)).astype(np.float32)
    c[::3] = dd_f32(4, 4000)[::3]                           # cancelling and ordinary addends
    r = ei.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        d = abs(Fraction(float(r[i])) - exact)
        for nb in (np.nextafter(r[i], np.float32(-np.inf)), np.nextafter(r[i], np.float32(np.inf))):
            assert d <= abs(Fraction(float(nb)) - exact), i


def dd_f32(seed, n):
    from tests import detdata as dd
    return dd.normal_f16(seed, (n,), 3.0).astype(np.float32) * np.float32(1.0009765)


def _gn_exact_cases():
    from tests.test_norm_exact_gpu import GN_EXACT
    return GN_EXACT


GN_EXACT_HOST = [c for c in _gn_exact_cases() if c[1] * c[2] <= 1 << 17]      # (the large ones: on the GPU only)


@pytest.mark.parametrize("case", GN_EXACT_HOST, ids=[f"hw{c[1]}_c{c[2]}_g{c[3]}_{c[5]}" for c in GN_EXACT_HOST])
def test_groupnorm_exact_inputs(oracle, case):
    """The closed formula gives the oracle's bits (two restatements: one of the kernel's order, one order-free), lies
    within the float64 bound, and every heavy position changes exactly one group's sums by the stated integers."""
    from tests import norm_edges as ne
    N, HW, Cc, G, silu, C1 = case
    geom = ne.gn_launch(N, HW, Cc, G, silu)
    x0, gamma, beta = ei.gn_base(N, HW, Cc, G)
    assert np.abs(x0.astype(np.float64)).max() <= 8
    s0, q0 = ei.gn_group_sums(x0, G)
    pos = ei.gn_heavy_positions(geom, C1)
    need = {"first_pixel", "last_pixel", "chunk_first", "chunk_last", "last_chunk_first", "last_pixel_lane",
            "group_first_channel", "group_last_channel"}
    if geom["cg"] % 8:
        need |= {"octet_leading_half", "octet_trailing_half"}
    if C1 is not None:
        need |= {"x_last_channel", "x2_first_channel"}
        assert pos["x_last_channel"][1] == C1 - 1 and pos["x2_first_channel"][1] == C1
    assert need <= set(pos)
    assert pos["first_pixel"][0] == 0 and pos["last_pixel"][0] == HW - 1
    assert pos["last_chunk_first"][0] == (geom["nchunk"] - 1) * geom["ppb"]
    assert pos["chunk_first"][0] % geom["ppb"] == 0 and (pos["chunk_last"][0] + 1) % geom["ppb"] in (0, HW % geom["ppb"])
    if "octet_leading_half" in pos:
        lo, hi = pos["octet_leading_half"][1], pos["octet_trailing_half"][1]
        assert lo % 8 == 0 and hi == lo + 7 and lo // geom["cg"] + 1 == hi // geom["cg"]
    for name, (p, ch) in [("base", (None, None))] + sorted(pos.items()):
        if name == "base":
            x = x0
        else:
            x, _, _, info = ei.gn_heavy(N, HW, Cc, G, p, ch)
            s, q = ei.gn_group_sums(x, G)
            assert (s - s0)[info["image"], info["group"]] == info["ds"] and np.count_nonzero(q - q0) == 1
            assert (q - q0)[info["image"], info["group"]] == info["dq"] and info["group"] == ch // geom["cg"]
        want, st = ei.gn_expected(x, gamma, beta, G)
        _, h = oracle.groupnorm_silu_quantize(x, gamma, beta, 1e-5, G, False, 1.0, 0.0)
        assert np.array_equal(want.view(np.uint16), h.view(np.uint16)), name
        # (the constant group has variance 0 -- mean / sigma is infinite: its bits are pinned, the bound is not for it)
        live = np.repeat(st["var"] > 0, Cc // G, axis=1)[:, None, :]
        assert (ne.within_norm_bound(want, ne.groupnorm64(x, gamma, beta, 1e-5, G)) | ~live).all(), name
    assert ei.gn_expected(x0, gamma, beta, G)[1]["var"][N - 1, 1] == 0           # the constant group


@pytest.mark.parametrize("C", [16, 32, 48, 96, 160, 320, 512, 960, 1024, 1168, 1536, 1920, 2032, 2048])
def test_layernorm_exact_inputs(oracle, C):
    from tests import norm_edges as ne
    x, gamma, beta, cols = ei.ln_heavy(C)
    g = ne.ln_geom(1, C)
    u = g["U"] // 2
    need = {0, C - 1} | {16 * (u * g["per"] + k) + d for k in range(g["per"] + 1) for d in (-1, 0)}
    if C >= 1024:
        need |= set(range(504, 520))
    assert {c for c in need if 0 <= c < C} <= set(cols)
    assert g["U"] == 1 or any(c % (16 * g["per"]) == 0 and 0 < c < C for c in cols)      # a unit boundary
    _, h = oracle.layernorm_quantize(x, gamma, beta, 1e-5, [])
    assert np.array_equal(ei.ln_expected_zero_mean(x[:1], gamma, beta).view(np.uint16), h[:1].view(np.uint16))
    assert ne.within_norm_bound(h, ne.layernorm64(x, gamma, beta, 1e-5)).all()
    for c in (0, 3, 4, -7):
        _, hc = oracle.layernorm_quantize(np.full((1, C), c, np.float16), gamma, beta, 1e-5, [])
        assert np.array_equal(ei.ln_expected_constant(c, C, gamma, beta).view(np.uint16), hc[0].view(np.uint16)), c
    assert np.array_equal(ei.ln_expected_constant(0, C, gamma, beta).view(np.uint16), beta.view(np.uint16))
    if C & (C - 1) == 0:            # rn(1 / C) exact: a constant row gives exactly beta
        assert np.array_equal(ei.ln_expected_constant(3, C, gamma, beta).view(np.uint16), beta.view(np.uint16))


def test_quantizer_edge_values_reach_ties_and_both_clamps():
    v = ei.qedge_values(2032)[0::2]
    for qp in ei.QEDGE_LN:
        assert all(ei.qedge_facts(v, *qp).values()), qp
    x = ei.qedge_values(33 * 64, seed=3)
    for qp in ei.QEDGE_RAW:
        assert all(ei.qedge_facts(x, *qp).values()), qp
    assert np.abs(ei.qedge_values(5000).astype(np.float64)).max() == 80
