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
    check_rescale_case(oracle, ei.rescale(kind, D, tkv), kind)


def check_rescale_case(oracle, c, kind, facts=True):
    _, ref64 = oracle.attention_f16(c["q"], c["k"], c["v"], c["heads"])
    scale = np.abs(c["v"].astype(np.float64)).max()
    assert np.abs(ref64 - c["expected"]).max() <= 1e-12 * scale
    if not facts:
        return
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


# ------------------------------------------------------------------------------------------ to_q + cross-attention
QATT = [(tkv, tq) for tkv in ei.QATT_KEY_COUNTS for tq in ei.QATT_QUERY_COUNTS]
QATT_IDS = [f"k{tkv}_q{tq}" for tkv, tq in QATT]


def attention_tolerance():
    from tests.test_attention_gpu import ATOL, RTOL
    return ATOL, RTOL


def check_toq(oracle, o, what):
    """oracle.qlinear on the operands, stored as W8 and unpacked from W4 and from W2, returns q bit for bit."""
    import torch
    from mixdq_amd.nn.utils import pack_w2, pack_w4, unpack_w2
    a, w, q = o["a"], o["w"], o["q"]
    B, T, K = a.shape
    assert K % 128 == 0 and T % 64 == 0 and w.shape == (q.shape[-1], K) and w.shape[0] % 128 == 0
    assert (o["scale"] == 1).all() and (o["bias0"] == 0).all()
    wt = torch.from_numpy(w)
    stored = {"W8": w, "W4": oracle.unpack_w4(pack_w4(wt).numpy()), "W2": unpack_w2(pack_w2(wt)).numpy()}
    for name, wi in stored.items():
        assert np.array_equal(wi, w), f"{what} {name}: the packed weights are other integers"
        got, acc = oracle.qlinear(a, wi, o["bias0"], o["scale"], None, return_acc=True)
        assert np.array_equal(got.view(np.uint16), q.view(np.uint16)), f"{what} {name}"
        assert np.array_equal(acc.astype(np.float64), q.astype(np.float64)), f"{what} {name}: accumulators"


def test_the_fused_launch_key_and_query_counts():
    assert ei.QATT_KEY_COUNTS == (1, 4, 5, 63, 64, 65, 77, 96, 97, 127, 128)
    assert ei.QATT_QUERY_COUNTS == (64, 192) and (ei.QATT_B, ei.QATT_HEADS) == (2, 4)
    assert ei.QATT_BLOCK * ei.QATT_B * ei.QATT_HEADS == 1024                       # eight K-tiles of 128
    assert set(ei.QATT_RESCALE_KEY_COUNTS) == {65, 77, 128} and all(n > 64 for n in ei.QATT_RESCALE_KEY_COUNTS)


@pytest.mark.parametrize("tkv,tq", QATT, ids=QATT_IDS)
def test_toq_selection_operands(oracle, tkv, tq):
    """The GEMM gives the hot key (W8, W4, W2); selection()'s own preconditions hold at four heads and 64 / 192
    queries (asserted inside the builder, restated from its stats); the oracle's attention on (q, k, v) is the hot
    value row; a reference that swaps two value rows is rejected at exactly the queries that address them."""
    o = ei.toq_operands("selection", tkv, tq)
    c = o["case"]
    a, w, hot, want, heads = o["a"], o["w"], c["hot"], c["expected"], c["heads"]
    B, D = a.shape[0], 64
    assert (B, heads, a.shape[2]) == (2, 4, 1024) and want.shape == (B, tq, heads * D)
    check_toq(oracle, o, f"selection k{tkv} q{tq}")
    st = c["stats"]
    assert st["min_gap"] >= 26 and 0 < st["min_hot"] <= st["max_hot"] <= 1000 and st["max_rest_ulps"] <= 1 / 16
    # the layout, restated: one 3 per (row, head block), at the hot key's column; sign codes below tkv, filler above
    assert set(np.unique(a)) == {0, 3} and ((a != 0).sum(axis=2) == heads).all()
    for b in range(B):
        for h in range(heads):
            c0 = 128 * (b * heads + h)
            assert np.array_equal(np.argmax(a[b, :, c0:c0 + 128], axis=1), hot[b, h])
            blk = w[:, c0:c0 + 128]
            ks = np.sign(c["k"][b, :, h * D:(h + 1) * D].astype(np.float64)).T
            assert np.array_equal(blk[h * D:(h + 1) * D, :tkv], ks)
            outside = np.delete(blk[:, :tkv], np.s_[h * D:(h + 1) * D], axis=0)
            assert (outside == 0).all() and (blk[:, tkv:] != 0).all() and set(np.unique(blk[:, tkv:])) <= {-2, -1, 1}
            reached = set(int(x) for x in hot[b, h])
            assert reached == set(range(tkv)) if tq >= tkv else required_keys(tkv) <= reached, (b, h)
    ATOL, RTOL = attention_tolerance()
    ref16, ref64 = oracle.attention_f16(o["q"], c["k"], c["v"], heads)
    assert np.array_equal(ref16.view(np.uint16), want.view(np.uint16))
    assert (np.abs(ref64 - want.astype(np.float64)) <= ATOL + RTOL * np.abs(ref64)).all()
    assert (np.abs(ref64 - want.astype(np.float64)) <= ei.ulp16(want) / 8).all()
    if tkv > 1:                      # the wrong variant: value rows j0 and j1 of (image 0, head 1) change places
        j0, j1 = (0, tkv - 1) if tkv < 64 or tkv == 64 else (63, 64)
        v2 = c["v"].copy()
        v2[0, [j0, j1], D:2 * D] = c["v"][0, [j1, j0], D:2 * D]
        wrong = ei.softmax_attention64(o["q"], c["k"], v2, heads).astype(np.float16)
        differs = (wrong.view(np.uint16) != want.view(np.uint16)).any(axis=2)              # [B, tq]
        assert np.array_equal(differs[0], np.isin(hot[0, 1], (j0, j1))) and differs[0].any() and not differs[1].any()
        other = wrong.view(np.uint16)[..., np.r_[0:D, 2 * D:4 * D]] == want.view(np.uint16)[..., np.r_[0:D, 2 * D:4 * D]]
        assert other.all()
    right = ei.softmax_attention64(o["q"], c["k"], c["v"], heads).astype(np.float16)
    assert np.array_equal(right.view(np.uint16), want.view(np.uint16))


@pytest.mark.parametrize("tkv,tq", QATT, ids=QATT_IDS)
def test_toq_zero_score_operands(oracle, tkv, tq):
    """q = 0 out of a GEMM that multiplies: dense non-zero rows against weight columns in cancelling pairs.  The
    oracle's attention gives 2048 / tkv; a reference that admits the clamped copy of the last key, or drops a key,
    is rejected by more than the ulp the GPU test allows."""
    ATOL, RTOL = attention_tolerance()
    o = ei.toq_operands("every_key_once", tkv, tq)
    c = o["case"]
    check_toq(oracle, o, f"every_key_once k{tkv} q{tq}")
    a, w = o["a"], o["w"]
    assert (a != 0).all() and (w != 0).all() and (o["q"] == 0).all() and not np.signbit(o["q"]).any()
    part = a[0, 0, :128].astype(np.int64) @ w[:, :128].astype(np.int64).T                    # one K-tile alone: exact 0 too,
    assert (part == 0).all() and (a[0, 0, :127].astype(np.int64) @ w[:, :127].astype(np.int64).T != 0).any()   # but not a split pair
    heads = c["heads"]
    _, ref64 = oracle.attention_f16(o["q"], c["k"], c["v"], heads)
    assert (np.abs(ref64 - c["expected"]) <= ATOL + RTOL * np.abs(ref64)).all()
    assert np.abs(ref64 - c["expected"]).max() <= 1e-12 * ei.PROBE / tkv
    assert required_keys(tkv) | {tkv - 1} <= set(int(x) for x in c["probes"].ravel())
    last = c["probes"] == tkv - 1                                                            # [B, C]
    assert last.any()
    # wrong variant 1: the clamped re-read of the last key admitted past the mask (one more key, a copy of the last)
    # (a single key: any number of copies of it give v -- there the selection family's distinct rows do the work)
    k2, v2 = (np.concatenate([x, x[:, -1:]], axis=1) for x in (c["k"], c["v"]))
    wrong = ei.softmax_attention64(o["q"], k2, v2, heads)
    off = np.abs(wrong - c["expected"]) > c["ulp"]
    assert off.all() or tkv == 1, "an admitted copy of the last key passes"
    assert np.allclose(wrong[:, 0][last], 2 * ei.PROBE / (tkv + 1)) and np.allclose(wrong[:, 0][~last], ei.PROBE / (tkv + 1))
    # wrong variant 2: key 0 dropped
    if tkv > 1:
        wrong = ei.softmax_attention64(o["q"], c["k"][:, 1:], c["v"][:, 1:], heads)
        assert (np.abs(wrong - c["expected"]) > c["ulp"]).all()
        assert (wrong[:, 0][c["probes"] == 0] == 0).all()
    if c["exact"]:
        o = ei.toq_operands("small_integers", tkv, tq)
        s = o["case"]
        check_toq(oracle, o, f"small_integers k{tkv} q{tq}")
        _, ref64 = oracle.attention_f16(o["q"], s["k"], s["v"], heads)
        assert np.abs(ref64 - s["mean"][:, None, :]).max() <= 1e-12 * max(1.0, np.abs(s["mean"]).max())
        assert (np.abs(ref64 - s["expected"].astype(np.float64)) <= ATOL + RTOL * np.abs(ref64)).all()
        vi = s["v"].astype(np.int64)
        assert np.array_equal(s["expected"][:, 0], (vi.sum(axis=1) / tkv).astype(np.float16))
        if tkv > 1:                  # two value rows exchanged between channels: another mean
            v2 = s["v"].copy()
            v2[:, 0] = s["v"][:, 0, ::-1]
            wrong = ei.softmax_attention64(o["q"], s["k"], v2, heads).astype(np.float16)
            assert (wrong.view(np.uint16) != s["expected"].view(np.uint16)).any()


QATT_RESCALE = [(kind, tkv) for kind in ei.RESCALE_KINDS[:-1] for tkv in ei.QATT_RESCALE_KEY_COUNTS]


@pytest.mark.parametrize("kind,tkv", QATT_RESCALE, ids=[f"{k}_k{n}" for k, n in QATT_RESCALE])
def test_toq_rescale_operands(oracle, kind, tkv):
    """q == 2 u exactly out of the GEMM (the noise stays in k); the facts of the kind hold as they do with noisy q."""
    assert ei.RESCALE_KINDS[-1] == "huge_values"               # the one kind whose q is no sign vector: chain only
    o = ei.toq_operands("rescale", tkv, 64, kind)
    c = o["case"]
    check_toq(oracle, o, f"rescale {kind} k{tkv}")
    assert set(np.unique(o["q"].astype(np.float64))) == {-2.0, 2.0} and (o["q"] == o["q"][:, :1]).all()
    assert c["facts"]["tile_max"].shape[-1] == 2 and c["heads"] == 4              # two key tiles
    a, w = o["a"], o["w"]
    assert set(np.unique(a)) == {0, 2} and ((a != 0).sum(axis=2) == 4).all()
    assert (w.reshape(w.shape[0], -1, 128)[:, :, ei.QATT_RESCALE_COLUMNS:] != 0).all()
    check_rescale_case(oracle, c, kind, facts=False)
    # The facts, for two tiles of which the second holds 1, 13 or 64 keys.  The noise of k moves a score by
    # sigma = alpha * 0.25 * log2(e) = 0.72 log2 units (q = 2 u has 64 entries of 2, the scale is 1 / 8); a tile's
    # maximum lies up to ~3.5 sigma above its level (64 draws), a single key's score within 3.5 sigma of it.
    sigma = 2 * 0.25 * ei.LOG2E
    tm = c["facts"]["tile_max"]
    d = np.median(tm[..., 1] - tm[..., 0])
    if kind in ("rise4", "rise40", "fall4", "fall40"):
        step = (40.0 if kind.endswith("40") else 4.0) * (1 if kind.startswith("rise") else -1)
        assert abs(d - step) <= 3.5 * sigma and np.sign(d) == np.sign(step), d        # alpha = 2^-|d| at the second tile
    elif kind == "late_dominant":
        if tkv - 2 >= 64:            # the dominant key (tkv - 2) in the second tile, behind a maximum of 50 in the first
            assert np.median(tm[..., 0]) >= 40 and d >= 40
        else:                        # 65 keys: it is key 63, the last of the FIRST tile; the second tile's one key
            assert np.median(tm[..., 0]) >= 90 and d <= -90      # underflows against it (P == 0, no rescale)
    else:
        sign = -1 if kind.endswith("negative") else 1
        assert np.abs(c["scores"] - 60.0 * sign).max() <= 0.5


def test_rescale_default_noise_is_unchanged():
    """q_noise defaults to the 0.25 the kinds always had: the default call and the explicit one give the same bits."""
    for kind in ("rise4", "equal_large"):
        c, d = ei.rescale(kind, 64, 77), ei.rescale.__wrapped__(kind, 64, 77, q_noise=0.25)
        assert all(np.array_equal(c[n].view(np.uint16), d[n].view(np.uint16)) for n in "qkv")
    assert (np.abs(ei.rescale("rise4", 64, 77)["q"].astype(np.float64)) != 2).any()


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
