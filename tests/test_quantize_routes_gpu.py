"""mixdq_quantize_f16_i8 over every route its strides take (cases, inputs and references: tests/quantize_routes.py;
tests/test_quantize_routes_host.py checks on the CPU that the table reaches what it claims).

Every case runs under both rounding variants and both activation widths -- the 12 instantiations of the three kernels
on every route they can take -- with an index-coded input (the result is the element's own logical index, so a
misplaced element is a mismatch with certainty) and a random one (bits of the oracle).  Each case asserts, from
mixdq_quantize_f16_i8_route and the device pointers of the call, that it ran on the route the table names: an
allocator that hands back another alignment fails the test instead of testing another kernel.  The cases the Python
binding cannot express, and the refusal, go through the C ABI into a sentinel-filled buffer with guard bytes
(tests/test_conv_geometry_gpu.py's helpers): what the call does not own keeps its bytes.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests import quantize_routes as qr
from tests.test_conv_geometry_gpu import Buf, SENTINEL, _stream, _sync_status, assert_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RUN_CASES = [c for c in qr.CASES if c["status"] == qr.OK]


@pytest.fixture(autouse=True, params=["A", "B"], ids=["fma", "mul_add"])
def epilogue_variant(request, monkeypatch):
    """Both roundings of the multiply-add (tests/test_ops_gpu.py's fixture)."""
    import mixdq_amd._C as C_
    monkeypatch.setattr(C_, "FLAGS", 1 if request.param == "B" else 0)
    return request.param


def scal(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def _i64(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def _on_route(C, c, xv, ov):
    got = qr.plan(C, xv, ov)
    assert got[:4] == (qr.OK, c["route"], c["rank"], c["sizes4"]), \
        f"{c['name']}: x at {xv.data_ptr():#x}, out at {ov.data_ptr():#x} give {got}"


def _raw_call(C, xv, ov, s_inv, zp, abits):
    """mixdq_quantize_f16_i8 on the views' own pointers, sizes and strides; returns the status after a sync."""
    nd = xv.dim()
    code = C._lib.mixdq_quantize_f16_i8(xv.data_ptr(), ov.data_ptr(), _i64(list(xv.shape)), _i64(list(xv.stride())),
                                        _i64(list(ov.stride())), nd, s_inv.data_ptr(), zp.data_ptr(),
                                        C.FLAGS | C._aflag(abits), _stream())
    return _sync_status(code)


def _owned_output(shape):
    """A sentinel-filled INT8 tensor of `shape` between guard bytes: (Buf, the tensor over its payload)."""
    buf = Buf(np.zeros(shape, np.int8), sentinel=True)
    return buf, buf.raw[buf.lo:buf.lo + buf.nb].view(torch.int8).view(shape)


def _run(C, c, backing, s_inv, zp, abits):
    """The case's launch on `backing`; returns the INT8 images of the view to compare, as (what, numpy array)."""
    if c["out"] is None:
        xv, _ = qr.views(c, DEV, backing)
        out = C.quantize_per_tensor_to_int8(xv, scal(s_inv), scal(zp), _abits=abits)
        _on_route(C, c, xv, out)                      # the pointers the binding passed
        assert tuple(out.shape) == tuple(xv.shape)
        # the binding's output is uninitialised memory, where an element the launch never wrote can hold anything,
        # the right value of an earlier run included: the same call once more into a sentinel-filled buffer
        buf, ob = _owned_output((out.numel(),))
        ov = ob.as_strided(out.shape, out.stride())
        _on_route(C, c, xv, ov)
        assert _raw_call(C, xv, ov, scal(s_inv), scal(zp), abits) == qr.OK and buf.untouched()
        return [("binding", out.cpu().numpy()), ("into a sentinel-filled buffer", ov.cpu().numpy())]
    buf, ob = _owned_output(c["out"]["backing"])
    xv, ov = qr.views(c, DEV, backing, out_backing=ob)
    _on_route(C, c, xv, ov)
    assert _raw_call(C, xv, ov, scal(s_inv), scal(zp), abits) == qr.OK
    full = torch.from_numpy(buf.value().copy())
    got = c["out"]["view"](full).clone().numpy()
    c["out"]["view"](full).fill_(SENTINEL)             # what is left is everything outside the output view
    assert buf.untouched() and bool((full == SENTINEL).all()), f"{c['name']}: bytes outside the output view were written"
    return [("into a view", got)]


@pytest.mark.parametrize("abits", [8, 4])
@pytest.mark.parametrize("c", RUN_CASES, ids=qr.case_id)
def test_index_coded(C, c, abits):
    """scale_inv 1, zero_point 0 on integer-valued halves: the result is (i % 251) - 125 at flat logical index i in both
    variants (no rounding occurs); A4: that value clamped to -113.  A read outside the view would show as +127."""
    backing, want = qr.index_coded(c["name"])
    for what, got in _run(C, c, backing, 1.0, 0.0, abits):
        assert_bits(got, qr.a4(want) if abits == 4 else want, f"{c['name']} A{abits} {what}")


@pytest.mark.parametrize("abits", [8, 4])
@pytest.mark.parametrize("c", RUN_CASES, ids=qr.case_id)
def test_random_equals_the_oracle(C, c, abits):
    want = qr.random_reference(c["name"], C.FLAGS & 1)
    for what, got in _run(C, c, qr.random_backing(c["name"]), qr.S_INV, qr.ZP, abits):
        assert_bits(got, qr.a4(want) if abits == 4 else want, f"{c['name']} A{abits} {what}")


@pytest.mark.parametrize("abits", [8, 4])
def test_refused_rank_writes_nothing(C, abits):
    """Six dimensions that do not collapse: MIXDQ_ERR_SHAPE from the planner and from the launch, the whole output
    still the sentinel; through the binding, RuntimeError with that status's string."""
    c = qr.BY_NAME["refused_rank6"]
    xv, _ = qr.views(c, DEV, qr.random_backing(c["name"]))
    buf, ob = _owned_output(tuple(xv.shape))
    assert qr.plan(C, xv, ob)[0] == qr.ERR_SHAPE
    assert _raw_call(C, xv, ob, scal(qr.S_INV), scal(qr.ZP), abits) == qr.ERR_SHAPE
    assert buf.still_sentinel()
    with pytest.raises(RuntimeError, match=re.escape(C._lib.mixdq_status_string(qr.ERR_SHAPE).decode())):
        C.quantize_per_tensor_to_int8(xv, scal(qr.S_INV), scal(qr.ZP), _abits=abits)
    torch.cuda.synchronize()


@pytest.mark.parametrize("abits", [8, 4])
def test_dense_deep_under_a_captured_graph(C, abits):
    """The four-loads-in-flight loop, captured once and replayed twice with the output zeroed in between: the eager
    run's bits, which are the oracle's."""
    c = qr.BY_NAME["dense_deep"]
    xv, _ = qr.views(c, DEV, qr.random_backing(c["name"]))
    s_inv, zp = scal(qr.S_INV), scal(qr.ZP)
    eager = C.quantize_per_tensor_to_int8(xv, s_inv, zp, _abits=abits)
    want = qr.random_reference(c["name"], C.FLAGS & 1)
    assert_bits(eager, qr.a4(want) if abits == 4 else want, "eager")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        C.quantize_per_tensor_to_int8(xv, s_inv, zp, _abits=abits)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = C.quantize_per_tensor_to_int8(xv, s_inv, zp, _abits=abits)
    _on_route(C, c, xv, out)
    for replay in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), f"replay {replay}"


@pytest.mark.parametrize("abits", [8, 4])
def test_rows_rank4_first_image_alone(C, abits):
    """Batch independence: the first image's sub-view alone equals the first slice of the whole."""
    c = qr.BY_NAME["rows_rank4"]
    xv, _ = qr.views(c, DEV, qr.random_backing(c["name"]))
    s_inv, zp = scal(qr.S_INV), scal(qr.ZP)
    whole = C.quantize_per_tensor_to_int8(xv, s_inv, zp, _abits=abits)
    _on_route(C, c, xv, whole)
    first = C.quantize_per_tensor_to_int8(xv[:1], s_inv, zp, _abits=abits)
    assert qr.plan(C, xv[:1], first)[:4] == (qr.OK, "rows", 3, (1,) + c["sizes4"][1:])
    assert torch.equal(first, whole[:1])
    want = qr.random_reference(c["name"], C.FLAGS & 1)
    assert_bits(whole, qr.a4(want) if abits == 4 else want, "whole")
