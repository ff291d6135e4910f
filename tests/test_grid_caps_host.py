"""tests/grid_caps.py on the CPU: the table is the census of the `grid_blocks(` call sites, every crossing case -- the new
ones and the ones existing tests run -- launches the instantiation its row claims on a grid at the cap with more items
than that grid has lanes, and the planted inputs of tests/test_grid_caps_gpu.py have what that file asserts about them.
Traced against the stand-in runtime of tests/launch_trace.py (mixdq_amd.build.build()'s objects); no GPU."""
import collections
import os
import re

import numpy as np
import pytest

from tests import grid_caps as gc
from tests import inpaint9_ref as I9
from tests import inpaint_ref as I

MIXDQ_OK = 0
GPU_FILE = os.path.join(gc.ROOT, "tests", "test_grid_caps_gpu.py")


@pytest.fixture(scope="module")
def traced():
    return gc.run_children()


def test_the_table_is_the_census_of_the_capped_launches():
    got, want = collections.Counter(gc.census()), collections.Counter(gc.table_census())
    assert got == want, {"without a row": sorted(map(str, got - want)), "rows without a call": sorted(map(str, want - got))}
    assert len(gc.census()) >= 20
    assert all(s["cases"] for s in gc.SITES)
    keys = [gc.case_key(c) for c in gc.CASES]
    assert len(set(keys)) == len(keys)


def test_the_cap_is_grid_blocks_own():
    text = open(os.path.join(gc.CSRC, "common.h")).read()
    assert "constexpr int kNumCU = %d;" % gc.NUM_CU in text
    assert "inline int grid_blocks(int64_t items, int per_cu = 8)" in text
    assert [gc.cap_items(p) for p in (8, 16, 32)] == [524288, 1048576, 2097152]


@pytest.mark.parametrize("c", gc.CASES, ids=gc.case_key)
def test_every_crossing_case_crosses(traced, c):
    status, launches = traced[gc.case_key(c)]
    assert status == MIXDQ_OK, (status, launches)
    grid = gc.cap_blocks(c["per_cu"])
    at = 0
    for symbol in c["symbols"]:                        # the capped launches, in the call's order
        found = [i for i in range(at, len(launches)) if f"::{symbol}(" in launches[i][0]]
        assert found, (symbol, [l[0] for l in launches])
        name, g, block, lds = launches[found[0]]
        assert g == [grid, 1, 1] and block == "256", (symbol, g, block)
        at = found[0] + 1
    lanes = grid * gc.LANES
    assert c["items"] > lanes, f"{c['items']} items fit one trip of {lanes} lanes"
    assert c["items"] % lanes != 0, "the last trip is a whole one"
    assert c["items"] < 2 ** 31                        # (nothing here is about 32-bit indices)


@pytest.mark.parametrize("c", gc.NEW, ids=gc.case_key)
def test_new_cases_divide_by_awkward_extents(c):
    for e in c["extents"]:
        assert e > 1 and e & (e - 1) != 0, f"extent {e} is a power of two"
    if c["batch_items"] is not None:
        assert c["batch_items"] < gc.cap_items(c["per_cu"]), "no batch boundary inside the first trip"
    text = open(GPU_FILE).read()
    assert re.search(r'gc\.by_test\("%s"\)\)\s*\ndef %s\(' % (c["test"], c["test"]), text), c["test"]


@pytest.mark.parametrize("c", [c for c in gc.CASES if c["kind"] == "old"], ids=gc.case_key)
def test_existing_rows_state_what_their_tests_run(c):
    path, test = c["test"].split("::")
    function = test.split("[")[0]
    assert re.search(r"^def %s\(" % function, open(os.path.join(gc.ROOT, path)).read(), re.M), c["test"]
    text = open(os.path.join(gc.ROOT, c["where"])).read()
    for needle in c["needles"]:
        assert needle in text, f"{c['where']} no longer says {needle!r}"


# ---- the planted inputs: what tests/test_grid_caps_gpu.py asserts about its own inputs, from the same generators -------
def _both(a, what):
    assert a.any() and not a.all(), f"{what}: all set or all clear"


def test_pixel_masks_straddle_the_second_trip():
    cap = gc.cap_items(8)
    i = np.arange(gc.PIXELS)
    s = gc.pattern(i, cap)
    _both(s[:cap], "first trip")
    _both(s[cap:], "second trip")
    assert s[cap - 61:cap + 53].all() and not s[cap + 53:cap + 200].any() and not s[cap - 62]
    _both(s[gc.H_ * gc.W_ - 50:gc.H_ * gc.W_ + 50], "around the batch boundary")
    assert gc.H_ * gc.W_ < cap
    for d in (gc.U8, gc.F16, gc.F32):                  # the values binarise to the decision, from both sides of the threshold
        v = np.asarray(gc.mask_values(s, i, d, np)).astype(gc.NP_DTYPE[d])
        assert np.array_equal(I.mask_set(v), s)
        assert len(np.unique(v[s])) >= 4 and len(np.unique(v[~s])) >= 4
    assert 128 in gc.mask_values(s, i, gc.U8, np)[s] and 127 in gc.mask_values(s, i, gc.U8, np)[~s]


def test_latent_planting_tells_nearest_from_any():
    cap = gc.cap_items(8)
    j = np.arange(gc.PIXELS)
    p, q, r, c = gc.latent_planting(j, cap)
    for part, what in ((slice(0, cap), "first trip"), (slice(cap, None), "second trip")):
        _both(p[part], f"nearest, {what}")
        _both((p | q)[part], f"any, {what}")
        assert (p[part] != (p | q)[part]).any(), f"{what}: ANY == NEAREST"
    assert r.min() == 1 and r.max() == 7 and c.min() == 1 and c.max() == 7
    assert len({(a, b) for a, b in zip(r[cap:cap + 49], c[cap:cap + 49])}) == 49      # every decoy position, in the second trip


def test_dilate_seed_leaves_room_at_both_radii():
    cap = gc.cap_items(32)
    H, W = gc.DIL_H, gc.DIL_W
    i = np.arange(2 * H * W)
    y, x = (i // W) % H, i % W
    s = gc.dilate_seed(i, y, x, cap).reshape(2, H, W)
    assert s.reshape(-1)[cap - 4:cap + 5].all()
    for r in (2, 40):
        d = gc.box_dilate(s, r).reshape(-1)
        _both(d[:cap], f"radius {r}, first trip")
        _both(d[cap:], f"radius {r}, second trip")
        assert d.sum() > s.sum()
    small = np.random.default_rng(5).random((2, 9, 11)) < 0.08  # the helper itself, against the definition
    for r in (0, 2, 40):
        assert np.array_equal(gc.box_dilate(small, r), I9.mask_dilate(small.astype(np.uint8) * 255, r) == 255)


def test_token_ids_are_a_permutation_code():
    a = next(c for c in gc.NEW if c["test"] == "test_embed_tokens")["args"]
    ids = gc.token_ids(np.arange(a["B"] * a["T"]), a["V"])
    assert ids.min() == 0 and ids.max() == a["V"] - 1 and len(np.unique(ids[:a["V"]])) == a["V"]
    assert len(np.unique(gc.image_code(np.arange(251), 0))) == 251
