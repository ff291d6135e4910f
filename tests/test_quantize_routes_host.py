"""tests/quantize_routes.py reaches what it is there for -- asked of the library (mixdq_quantize_f16_i8_route, the
planner mixdq_quantize_f16_i8 itself calls: host code, no GPU), with CPU buffers of the alignment the cases name -- and
its inputs can tell a wrong result from a right one.  No launch here; tests/test_quantize_routes_gpu.py runs the cases."""
import ctypes

import numpy as np
import pytest
import torch

from tests import quantize_routes as qr


@pytest.fixture(scope="module")
def C():
    import mixdq_amd._C as C_
    return C_


@pytest.mark.parametrize("c", qr.CASES, ids=qr.case_id)
def test_case_reaches_its_route(C, c):
    xv, ov = qr.views(c)
    status, route, rank, sizes4, blocks = qr.plan(C, xv, ov)
    assert status == c["status"]
    if status != qr.OK:
        return
    assert (route, rank, sizes4) == (c["route"], c["rank"], c["sizes4"])
    assert int(np.prod(sizes4, dtype=np.int64)) == xv.numel()
    items = qr.work_items(c)
    assert 1 <= blocks <= qr.GRID_CAP_BLOCKS
    lanes = blocks * 256
    if c.get("deep"):
        nvec = xv.numel() >> 3
        assert nvec > 3 * lanes and xv.numel() > qr.DEEP_MIN_NUMEL
        # every lane one four-deep trip, then lanes below `rest` one single trip more, then the tail
        rest = nvec - 4 * lanes
        assert 0 < rest < lanes and xv.numel() % 8 != 0
    elif route == "dense":
        assert (xv.numel() >> 3) <= 3 * lanes               # the four-deep loop is not entered
    if c["name"] == "dense_just_below":
        assert lanes < (xv.numel() >> 3) <= 3 * lanes        # ... the second trip of the single loop is
    if c.get("two_trips"):
        assert items > lanes and blocks == qr.GRID_CAP_BLOCKS
    elif route != "dense":
        assert items <= lanes


def test_table_holds_every_route_at_every_rank():
    """Fails when a case is deleted: each route with each collapsed rank it can have, the refusal, both thresholds
    from both sides, both alignment gates and the raw-ABI output views."""
    have = {(c["route"], c["rank"]) for c in qr.CASES if c["status"] == qr.OK}
    assert have == qr.ROUTE_RANKS
    assert [c["name"] for c in qr.CASES if c["status"] == qr.ERR_SHAPE] == ["refused_rank6"]
    assert {c["name"] for c in qr.CASES if c.get("deep")} == {"dense_deep"}
    assert {(c["route"]) for c in qr.CASES if c.get("two_trips")} == {"rows", "scalar"}
    assert any(c.get("x_mod16") == 2 and c["route"] == "scalar" and c["rank"] == 1 for c in qr.CASES)
    assert any(c.get("out_mod8") == 4 and c["route"] == "scalar" for c in qr.CASES)
    assert sum(c["out"] is not None for c in qr.CASES) == 3
    assert any(c.get("overlapping") for c in qr.CASES)
    assert len(qr.CASES) == 16


@pytest.mark.parametrize("name", ["rows_rank4", "rows_rank4_offset", "scalar_rank4"])
def test_rank4_strides_make_an_index_swap_visible(name):
    """From the table alone: the four input strides are pairwise different, and every outer one differs from the
    output's (the inner stride is 1 on both sides) -- xs[i] <-> xs[j], os for xs, or size[i] for size[j] in a kernel's
    index arithmetic then addresses another element."""
    c = qr.BY_NAME[name]
    xv, ov = qr.views(c)
    xs, os_, sz = list(xv.stride()), list(ov.stride()), list(xv.shape)
    assert c["rank"] == 4 and len(xs) == 4 and xs == sorted(xs, reverse=True) and tuple(sz) == c["sizes4"]
    assert len(set(xs)) == 4 and len(set(os_)) == 4 and len(set(sz)) == 4
    assert all(xs[i] != os_[i] for i in range(3)) and xs[3] == os_[3] == 1
    assert all(s > 1 for s in sz)


@pytest.mark.parametrize("c", qr.CASES, ids=qr.case_id)
def test_index_coded_input_is_what_the_table_says(c):
    b, want = qr.index_coded(c["name"])
    bt = torch.from_numpy(b)
    v = c["view"](bt)
    assert np.array_equal(v.to(torch.int8).numpy(), want)
    assert b.dtype == np.float16 and want.dtype == np.int8
    if c.get("overlapping"):
        assert np.array_equal(b.reshape(-1).astype(np.int64), np.arange(b.size) % 251 - 125)
        return
    assert np.array_equal(want.reshape(-1).astype(np.int64), np.arange(want.size) % 251 - 125)
    # everything outside the view holds 127.0, which no viewed element does
    assert want.max() <= 125 and int((b == 127.0).sum()) == b.size - want.size
    if want.size > 200:                # both sides of the A4 clamp
        assert (want > qr.A4_MAX).any() and (want < qr.A4_MAX).any()


@pytest.mark.parametrize("c", qr.CASES, ids=qr.case_id)
def test_random_reference_can_tell_a_wrong_result(c, oracle):
    """The reference image alone, both variants: at most 1 % saturated, at least 200 distinct values, elements on both
    sides of the A4 clamp.  (One-element cases: the element does not saturate.)"""
    for variant in (0, 1):
        want = qr.random_reference(c["name"], variant)
        sat = np.count_nonzero((want == -128) | (want == 127))
        assert sat <= qr.RANDOM_CONDITIONS["max_saturated"] * want.size, (sat, want.size)
        if want.size < qr.RANDOM_CONDITIONS["min_distinct"]:
            assert c["name"].startswith("rank0_and_ones") and want.size == 1
            continue
        assert np.unique(want).size >= qr.RANDOM_CONDITIONS["min_distinct"], np.unique(want).size
        assert (want > qr.A4_MAX).any() and (want < qr.A4_MAX).any() and (qr.a4(want) == qr.A4_MAX).any()


def test_route_export_validates_like_the_launch(C):
    """The statuses the launch gives before launching: a negative size or stride, a null pointer with elements to
    move, ndim out of range; no element: MIXDQ_OK, route none, nothing to launch."""
    arr = lambda *v: (ctypes.c_int64 * len(v))(*v)
    f = C._lib.mixdq_quantize_f16_i8_route
    assert f(arr(4), arr(1), arr(1), 9, 64, 64, None, None, None, None) == 1
    assert f(arr(4), arr(1), arr(1), -1, 64, 64, None, None, None, None) == 1
    assert f(arr(-4), arr(1), arr(1), 1, 64, 64, None, None, None, None) == 1
    assert f(arr(4), arr(-1), arr(1), 1, 64, 64, None, None, None, None) == 1
    assert f(arr(4), arr(1), arr(1), 1, None, 64, None, None, None, None) == 1
    assert f(arr(4), arr(1), arr(1), 1, 64, 64, None, None, None, None) == 0          # every output may be null
    assert C.quantize_route([2, 0, 4], [4, 4, 1], [4, 4, 1], 0, 0) == (0, "none", 0, (1, 1, 1, 0), 0)
    assert C.quantize_route([16], [1], [1], 64, 64) == (0, "dense", 1, (1, 1, 1, 16), 1)
    assert C.quantize_route([16], [1], [1], 64, 68)[:2] == (0, "scalar")               # output 4 off 8
    assert C.quantize_route([16], [1], [1], 72, 64)[:2] == (0, "scalar")               # input 8 off 16
