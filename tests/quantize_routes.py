"""Case table of the per-tensor quantize launch (mixdq_quantize_f16_i8, csrc/quantize.hip) over every route its
strides take (tests/test_quantize_routes_host.py checks on the CPU that each case reaches what it is there for;
tests/test_quantize_routes_gpu.py runs them).

The entry point sorts the dimensions by input stride, drops size-1 dimensions, collapses mergeable neighbours to a
rank m <= 4 and launches one of three kernels -- dense (linear on both sides, 16 bytes a lane-step, four loads in
flight), rows (inner run contiguous on both sides and vectorisable by 8) or scalar (one element a lane-step) -- on a
grid capped at 8 blocks per CU.  None of that is restated here: every case carries the route, rank and collapsed sizes
it exists to reach, and the tests ask mixdq_quantize_f16_i8_route -- the planner the launch itself calls -- whether
the buffers actually passed get there.

A case names a contiguous FP16 backing buffer and the view taken of it.  `out` is None where the Python binding can
express the call (it allocates torch.empty_like(view, dtype=int8)); otherwise the case goes through the C ABI into a
view of a wider INT8 buffer.  Two inputs per case:

  index-coded   the element at flat logical index i of the view is (i % 251) - 125, the rest of the backing buffer
                127.0 (a value no viewed element has); scale_inv 1, zero_point 0: the result is (i % 251) - 125
                whatever the rounding variant, and a misplaced or misread element is a mismatch with certainty (251
                is prime and larger than every inner run here).  A view that overlaps itself (`broadcast`) cannot hold
                one code per logical index: there the backing buffer is coded by ITS flat index.
  random        FP16 values uniform over [-11.8, 12.2] over the whole backing buffer, scale_inv 10.5, zero_point -3.0,
                compared with the oracle bit for bit.  The image spans -127 .. 125 without saturating, so that every
                case of 600 elements or more meets RANDOM_CONDITIONS.  (A Gaussian of standard deviation 2.0 under
                this quantizer does not: its image has a standard deviation of 21 steps around -3, the A4 clamp at -113
                lies 5.2 sigma out and 200 distinct values need both tails to 4.7 sigma -- 4 million elements reach
                neither.)

Plain Python + numpy + torch on the CPU; imports without a GPU and without the built library.
"""
import functools

import numpy as np
import torch

from tests import detdata as dd

GRID_CAP_BLOCKS = 256 * 8                 # grid_blocks (csrc/common.h): kNumCU * 8 blocks of 256 lanes
GRID_CAP_LANES = GRID_CAP_BLOCKS * 256    # 524 288 work items: more than that and a lane makes a second trip
DEEP_MIN_NUMEL = 8 * 3 * GRID_CAP_LANES   # 12 582 912: beyond it the dense kernel's four-loads-in-flight loop runs
OK, ERR_SHAPE = 0, 9                      # include/mixdq_hip.h
A4_MAX = -113                             # MIXDQ_FLAG_A4_0: the INT8 image clamped to [-128, -113]
CODE_MOD, CODE_OFF, OUTSIDE = 251, 125, 127.0
S_INV, ZP = 10.5, -3.0
UNIFORM_LO, UNIFORM_HI = -11.8, 12.2
# the random input's reference image, per case: at most 1 % saturated, at least 200 distinct values, and elements on
# both sides of the A4 clamp (cases of fewer than 200 elements -- rank0_and_ones_* have one -- cannot have the last
# two: for them the element must not saturate)
RANDOM_CONDITIONS = dict(max_saturated=0.01, min_distinct=200)

_DEEP = 8 * (4 * GRID_CAP_LANES + GRID_CAP_LANES // 2 + 3) + 5       # 18 874 397
_R4, _R6, _TT = (3, 5, 7, 64), (2, 3, 4, 5, 6, 16), (2, 1100, 2056)


def _case(name, backing, view, route, rank, sizes4, why, out=None, status=OK, seed=0, **props):
    return dict(name=name, backing=backing, view=view, route=route, rank=rank, sizes4=sizes4, why=why, out=out,
                status=status, seed=7000 + seed, **props)


CASES = [
    _case("dense_deep", (_DEEP,), lambda b: b, "dense", 1, (1, 1, 1, _DEEP),
          "every lane one four-deep trip, half the lanes one single trip more, a 5-element tail",
          seed=1, deep=True),
    _case("dense_just_below", (8 * GRID_CAP_LANES + 24,), lambda b: b, "dense", 1, (1, 1, 1, 8 * GRID_CAP_LANES + 24),
          "second trip of the single loop only; the four-deep loop not entered", seed=2),
    _case("dense_misaligned_in", (600001,), lambda b: b[1:], "scalar", 1, (1, 1, 1, 600000),
          "contiguous, base 2 bytes off 16: leaves the dense kernel; more than one grid-stride trip",
          seed=3, two_trips=True, x_mod16=2),
    _case("rows_rank4", _R4, lambda b: b[:, :4, :6, :48], "rows", 4, (3, 4, 6, 48),
          "all of size[0..2] > 1, all three outer input strides differ from the output's", seed=4),
    _case("rows_rank4_offset", _R4, lambda b: b[:, :4, :6, 8:56], "rows", 4, (3, 4, 6, 48),
          "base advanced by a multiple of 16 bytes", seed=4),
    _case("scalar_rank4", _R4, lambda b: b[:, :4, :6, :44], "scalar", 4, (3, 4, 6, 44),
          "inner run no multiple of 8", seed=4),
    _case("rows_rank3_from_6", _R6, lambda b: b[:, :, :, :, :5, :8], "rows", 3, (1, 120, 5, 8),
          "a rank-6 tensor that collapses", seed=5),
    _case("refused_rank6", _R6, lambda b: b[:, :2, :3, :4, :5, :8], None, None, None,
          "a rank that does not collapse: MIXDQ_ERR_SHAPE, nothing written", status=ERR_SHAPE, seed=5),
    _case("broadcast", (40, 64), lambda b: b[:, None, :].expand(40, 3, 64), "scalar", 3, (1, 40, 64, 3),
          "input inner stride 0, output inner stride 64", seed=6, overlapping=True),
    _case("rows_two_trips", _TT, lambda b: b[..., :2048], "rows", 2, (1, 1, 2200, 2048),
          "more than 524 288 work items", seed=7, two_trips=True),
    _case("scalar_two_trips", _TT, lambda b: b[..., :2047], "scalar", 2, (1, 1, 2200, 2047),
          "more than 524 288 work items", seed=7, two_trips=True),
    # channels-last (2, 8, 6, 10): the backing buffer is its NHWC storage
    _case("chan_last_split_into_nchw", (2, 6, 10, 8), lambda b: b.permute(0, 3, 1, 2)[:, :5], "scalar", 3, (1, 2, 60, 5),
          "output strides ordered unlike the input's", seed=8,
          out=dict(backing=(2, 5, 6, 10), view=lambda o: o)),
    _case("into_column_range", (40, 64), lambda b: b, "rows", 2, (1, 1, 40, 64),
          "output row stride 200", seed=9, out=dict(backing=(40, 200), view=lambda o: o[:, 64:128])),
    _case("into_unaligned_column_range", (40, 64), lambda b: b, "scalar", 2, (1, 1, 40, 64),
          "output base 4 bytes off 8: leaves the rows kernel", seed=9,
          out=dict(backing=(40, 200), view=lambda o: o[:, 60:124]), out_mod8=4),
    _case("rank0_and_ones_0d", (1,), lambda b: b.reshape(()), "dense", 1, (1, 1, 1, 1), "tail only", seed=10),
    _case("rank0_and_ones_111", (1,), lambda b: b.reshape(1, 1, 1), "dense", 1, (1, 1, 1, 1), "tail only", seed=10),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# what the table must hold: every route with each collapsed rank it can have
ROUTE_RANKS = {("dense", 1), ("rows", 2), ("rows", 3), ("rows", 4),
               ("scalar", 1), ("scalar", 2), ("scalar", 3), ("scalar", 4)}


def case_id(c):
    return c["name"]


# ------------------------------------------------------------------------------------------------ buffers
def alloc(shape, dtype, device="cpu", fill=None):
    """A contiguous tensor whose base is on a 64-byte boundary (asserted: a case's alignment is part of the case)."""
    n = int(np.prod(shape, dtype=np.int64))
    size = torch.empty((), dtype=dtype).element_size()
    raw = torch.empty(n * size + 64, dtype=torch.uint8, device=device)
    off = (-raw.data_ptr()) % 64
    t = raw[off:off + n * size].view(dtype).view(shape)
    assert t.data_ptr() % 64 == 0 and t.is_contiguous()
    if fill is not None:
        t.fill_(fill)
    return t


def work_items(c):
    """Lane-steps of the launch: 8-element pieces on the dense and rows routes, elements on the scalar one."""
    n = int(np.prod(c["sizes4"], dtype=np.int64))
    return n if c["route"] == "scalar" else n >> 3


def plan(C, xv, ov):
    """(status, route, rank, sizes4, blocks) from the library for this input view and output view."""
    nd = xv.dim()
    return C.quantize_route(list(xv.shape) if nd else [1], list(xv.stride()) if nd else [1],
                            list(ov.stride()) if nd else [1], xv.data_ptr(), ov.data_ptr())


def views(c, device="cpu", x_backing=None, out_backing=None):
    """The input view and the output view of a case on freshly aligned buffers (`x_backing`: a host array to copy in;
    `out_backing`: the tensor to take the output view of, where the caller owns the output).  Returns (xv, ov); ov is a
    stand-in with the binding's strides (torch.empty_like(xv, dtype=int8)) where the binding allocates the output."""
    b = alloc(c["backing"], torch.float16, device)
    if x_backing is not None:
        b.copy_(torch.from_numpy(x_backing))
    xv = c["view"](b)
    assert xv.data_ptr() % 16 == c.get("x_mod16", 0), c["name"]
    if c["out"] is None:
        ov = torch.empty_like(xv, dtype=torch.int8) if out_backing is None else out_backing
    else:
        ov = c["out"]["view"](alloc(c["out"]["backing"], torch.int8, device) if out_backing is None else out_backing)
    assert tuple(ov.shape) == tuple(xv.shape) and ov.data_ptr() % 8 == c.get("out_mod8", 0), c["name"]
    return xv, ov


# ------------------------------------------------------------------------------------------------ inputs
def codes(n):
    """(i % 251) - 125 for i < n, int8."""
    return ((torch.arange(n, dtype=torch.int32) % CODE_MOD) - CODE_OFF).to(torch.int8)


@functools.lru_cache(maxsize=None)
def index_coded(name):
    """(backing FP16 array, expected INT8 image of the view) of the index-coded input; built once, read only."""
    c = BY_NAME[name]
    b = torch.full(c["backing"], OUTSIDE, dtype=torch.float16)
    if c.get("overlapping"):
        b.copy_(codes(b.numel()).view(c["backing"]))
        want = c["view"](b).to(torch.int8).contiguous()
    else:
        v = c["view"](b)
        want = codes(v.numel()).view(v.shape)
        v.copy_(want)
    want = want.numpy()
    want.setflags(write=False)
    return b.numpy(), want


@functools.lru_cache(maxsize=None)
def random_backing(name):
    c = BY_NAME[name]
    return dd.f16(c["seed"], c["backing"], UNIFORM_LO, UNIFORM_HI)


@functools.lru_cache(maxsize=None)
def random_reference(name, variant):
    """oracle.quantize of the view's host copy under `variant` (0 FMA, 1 multiply-round-add); built once."""
    from oracle import oracle as O
    c = BY_NAME[name]
    want = O.quantize(c["view"](torch.from_numpy(random_backing(name))).numpy(), S_INV, ZP, variant)
    want.setflags(write=False)
    return want


def a4(q8):
    """The A4 image: the INT8 one clamped to [-128, -113] (tests/test_a4_gpu.py)."""
    return np.minimum(q8, A4_MAX).astype(np.int8)
