"""CPU checks of tests/conv_geometry.py: the cases cover what they claim, the numpy reference equals the C oracle on
every case and torch on the zero-point term, and the FP16 expectations of the extended exact_inputs.conv2d hold."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_geometry as cg
from tests import exact_inputs as ei
from tests import tile_edges as te

INT_CASES = cg.INT8_CASES + cg.W4_CASES


def test_every_geometry_tile_channel_class_and_stride_remainder_occurs():
    for cases, channels, tiles in ((cg.INT8_CASES, cg.C_INT8, cg.TILES), (cg.W4_CASES, cg.C_W4, cg.TILES),
                                   (cg.F16_CASES, cg.C_F16, cg.TILES_F16)):
        geoms = {(c["R"], c["S"], c["stride"], c["pad"]) for c in cases}
        assert geoms >= set(cg.GEOMETRIES)
        assert {c["cfg"] for c in cases} == set(tiles)
        assert {c["C"] for c in cases} == set(channels)
        for g in geoms:
            mine = [c for c in cases if (c["R"], c["S"], c["stride"], c["pad"]) == g]
            assert {c["C"] for c in mine} == set(channels)
            assert {c["image"] for c in mine} == {"tiny", "ragged", "full"}
            assert {c["n"] for c in mine} == {1, 3}
            rem = {cg.stride_remainder(c["H"], c["R"], c["stride"], c["pad"]) != 0 for c in mine}
            assert rem == ({False, True} if g[2] > 1 else {False}), g
            assert all(c["H"] <= 16 and c["W"] <= 16 and c["P"] >= 1 and c["Q"] >= 1 for c in mine)
    assert {(c["R"], c["S"], c["stride"], c["pad"]) for c in cg.F16_CASES} >= set(cg.REFUSED)
    assert all(g[3] < g[0] and g[3] < g[1] for g in cg.GEOMETRIES)
    assert all(g[3] >= g[0] or g[3] >= g[1] for g in cg.REFUSED)
    assert cg.GEOMETRIES[-1] == (3, 3, 1, 1)
    assert {c["residual"] for c in cg.INT8_CASES} == {"", "full", "image"} and {c["bias"] for c in INT_CASES} == {False, True}
    assert all(c["cfg"] == 0 for c in cg.INT8_CASES if c["C"] in cg.C_GENERIC)
    # the whole GPU file stays small: INT8 and W4 cases run under both epilogue variants
    assert 2 * len(INT_CASES) + len(cg.F16_CASES) <= 330


def test_tiles_cover_every_value_of_every_gather_parameter():
    for rows, tiles in ((cg.IGEMM_GATHER, cg.TILES), (cg.F16_GATHER, cg.TILES_F16)):
        assert tiles[0] == 0 and set(tiles[1:]) <= set(rows)
        for i in range(len(next(iter(rows.values())))):
            assert {rows[c][i] for c in tiles[1:]} == {v[i] for v in rows.values()}, f"parameter {i}"
    assert {cg.IGEMM_GATHER[c][1] for c in cg.TILES[1:]} == {64, 128}            # BK
    assert {cg.IGEMM_GATHER[c][6] for c in cg.TILES[1:]} == {False, True}        # the four-phase loop
    assert all(c["K"] in (cg.tile_bn(c["cfg"]) + 4, 2 * cg.tile_bn(c["cfg"]) - 4) for c in INT_CASES)
    assert all(c["K"] in (cg.tile_bn(c["cfg"], te.F16) + 4, 2 * cg.tile_bn(c["cfg"], te.F16) - 4) for c in cg.F16_CASES)


@pytest.mark.parametrize("case", INT_CASES, ids=[cg.case_id(c) for c in INT_CASES])
def test_border_classes_met(case):
    """By the geometry alone: a padded conv has a top and a left border; it has a bottom (right) border where the
    stride remainder leaves padding rows (columns) in reach, (H + 2 pad - R) % stride < pad.  The window intersection
    must find a non-interior class on each such side -- and no class outside the table's non-empty rectangles."""
    R, S, stride, pad, H, W = (case[k] for k in ("R", "S", "stride", "pad", "H", "W"))
    met = cg.border_classes(R, S, stride, pad, H, W)
    assert all(0 <= rlo <= rhi < R and 0 <= slo <= shi < S for rlo, rhi, slo, shi in met)
    assert all(rlo <= pad and slo <= pad for rlo, _, slo, _ in met)
    assert any(c[0] > 0 for c in met) == (pad > 0) and any(c[2] > 0 for c in met) == (pad > 0)
    bottom, right = (H + 2 * pad - R) % stride < pad, (W + 2 * pad - S) % stride < pad
    assert any(c[1] < R - 1 for c in met) == bottom and any(c[3] < S - 1 for c in met) == right
    if case["image"] == "full":
        assert (0, R - 1, 0, S - 1) in met, "no interior pixel"
        if pad:
            assert bottom and right, "the full image must have all four borders"
            assert any(c[0] > 0 and c[2] > 0 for c in met) and any(c[1] < R - 1 and c[3] < S - 1 for c in met)
    if case["image"] == "tiny" and pad:
        assert any(c[0] > 0 and c[1] < R - 1 for c in met) or R <= 2, "no pixel on the first and the last border at once"


@pytest.mark.parametrize("g", cg.GEOMETRIES + cg.REFUSED, ids=str)
def test_output_shape_equals_torch(g):
    R, S, stride, pad = g
    for _, n, H, W in cg.images(*g):
        y = F.conv2d(torch.zeros(n, 1, H, W), torch.zeros(1, 1, R, S), stride=stride, padding=pad)
        assert tuple(y.shape[2:]) == cg.out_hw(H, W, R, S, stride, pad)


@pytest.mark.parametrize("case", INT_CASES, ids=[cg.case_id(c) for c in INT_CASES])
def test_reference_equals_oracle_and_torch(oracle, case):
    d = cg.inputs(case)
    R, S, stride, pad, n, H, W, K = (case[k] for k in ("R", "S", "stride", "pad", "n", "H", "W", "K"))
    wsum = cg.wsum_of(d["w"])
    if case["form"] == "w4":
        from mixdq_amd.nn.utils import pack_w4
        assert d["w"].min() == -8 and d["w"].max() == 7
        assert np.array_equal(oracle.unpack_w4(pack_w4(torch.from_numpy(d["w"])).numpy()), d["w"])
    else:
        assert d["x"].min() == -128 and d["x"].max() == 127
    # zero-point term: float64 conv of a constant-zp image with the tap sums, rounded
    b0 = cg.zero_point_term(wsum, cg.ZP, H, W, stride, pad)
    t64 = F.conv2d(torch.full((1, 1, H, W), cg.ZP, dtype=torch.float64),
                   torch.from_numpy(wsum).double().reshape(K, 1, R, S), stride=stride, padding=pad)
    assert np.array_equal(b0, t64[0].permute(1, 2, 0).numpy().astype(np.float32))
    assert np.array_equal(np.broadcast_to(b0[None], (n,) + b0.shape), oracle.zp_propagate(wsum, cg.ZP, n, H, W, stride, pad))
    bias0 = b0[0, 0] if pad == 0 else None
    for variant in (0, 1):
        want, acc = oracle.qconv2d(d["x"], d["w"], d["scale"], wsum if pad else None, cg.ZP, bias0, d["bias"], stride,
                                   pad, variant, return_acc=True)
        assert np.array_equal(acc, cg.accumulators(case))
        got = cg.reference(case, variant, with_residual=False)
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), f"variant {variant}"
        if d["residual"] is not None:
            r = d["residual"] if case["residual"] == "full" else np.broadcast_to(d["residual"][:, None, None, :], want.shape)
            assert np.array_equal(cg.reference(case, variant).view(np.uint16), oracle.add_f16(want, r).view(np.uint16))


def test_conv2d_exact_inputs_take_a_rectangle_and_keep_the_square_data():
    sq = ei.conv2d(3, 8, 7, 9, 12, 3, 1, 0, True)
    x = ei._ints16(ei._seed(3, 8, 7, 9, 12, 3, 1, 0, 0), (3, 8, 7, 9), 4)
    assert np.array_equal(sq["x"], x) and sq["w"].shape == (12, 8, 3, 3)
    for c in cg.F16_CASES[::7]:
        e = cg.f16_case(c)
        assert e["w"].shape == (c["K"], c["C"], c["R"], c["S"]) and e["expected"].shape == (c["n"], c["K"], c["P"], c["Q"])
        y = F.conv2d(torch.from_numpy(e["x"]).double(), torch.from_numpy(e["w"]).double(),
                     None if e["bias"] is None else torch.from_numpy(e["bias"]).double(), stride=c["stride"], padding=c["pad"])
        if e["residual"] is None:
            assert np.array_equal(y.numpy().astype(np.float16), e["expected"])
