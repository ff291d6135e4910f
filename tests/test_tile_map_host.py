"""tests/tile_map.py on the CPU: the numpy restatement of the workgroup -> tile map is a bijection onto the tile grid,
every kernel family's cases reach the map's three branches, the table of sites is the census of the run formula in
csrc/, and the index-coded operands name their tiles.  No GPU, no built library."""
import os

import numpy as np
import pytest

from tests import tile_edges as te
from tests import tile_map as tm


def test_the_restatement_is_a_bijection_onto_the_tile_grid():
    """All tiles_m, tiles_n <= 40, gm in 1..64: the sequence visits every tile once, the runs partition it, and the
    workgroups of a launch map one to one onto it.  (gm >= tiles_m gives one super-row: checked once per tiles_m.)"""
    for tiles_m in range(1, 41):
        for tiles_n in range(1, 41):
            tiles = tiles_m * tiles_n
            r = tm.runs(tiles)
            assert r[0][0] == 0 and r[-1][1] == tiles and all(r[i][1] == r[i + 1][0] for i in range(7))
            assert max(e - s for s, e in r) - min(e - s for s, e in r) <= 1
            seqs = np.array([tm.seq_of(b, tiles) for b in range(tiles)])
            assert np.array_equal(np.sort(seqs), np.arange(tiles))
            for gm in [g for g in range(1, 65) if g < tiles_m] + [64]:
                s = tm.sequence(tiles_m, tiles_n, gm)
                assert s.shape == (tiles, 2)
                flat = s[:, 0] * tiles_n + s[:, 1]
                assert np.array_equal(np.sort(flat), np.arange(tiles)), (tiles_m, tiles_n, gm)
                # super-rows in order, m fastest inside
                assert np.array_equal(s[:, 0] // gm, np.sort(s[:, 0] // gm))


@pytest.mark.parametrize("tiles_m,tiles_n,gm", [(9, 3, 8), (11, 1, 8), (3, 3, 2), (3, 2, 1), (18, 2, 8), (37, 5, 8)])
def test_tile_of_and_the_persistent_form_cover_the_grid_once(tiles_m, tiles_n, gm):
    tiles = tiles_m * tiles_n
    got = [tm.tile_of(b, tiles_m, tiles_n, gm) for b in range(tiles)]
    assert sorted(got) == [(m, n) for m in range(tiles_m) for n in range(tiles_n)]
    for cap in (None, 8, 16):
        grid = tm.persistent_grid(tiles, cap=cap)
        assert grid % 8 == 0 and grid >= 8 and grid < tiles + 8
        seen = []
        for b in range(grid):
            k = 0
            while (s := tm.persistent_seq(b, k, grid, tiles)) is not None:
                seen.append(s)
                k += 1
        assert sorted(seen) == list(range(tiles)), (cap, grid)


def test_hand_worked_maps():
    """9 x 1 tiles, gm 8: the sequence is m = 0 .. 8; XCD 0 owns two tiles (0, 1), the others one each: workgroup 8 is
    XCD 0's second and computes m-tile 1, workgroup 1 (XCD 1's first) m-tile 2.  3 x 2 tiles at gm = 2: super-rows
    {0, 1} and {2}: (0,0) (1,0) (0,1) (1,1) (2,0) (2,1)."""
    assert [tm.tile_of(b, 9, 1)[0] for b in range(9)] == [0, 2, 3, 4, 5, 6, 7, 8, 1]
    assert tm.sequence(3, 2, 2).tolist() == [[0, 0], [1, 0], [0, 1], [1, 1], [2, 0], [2, 1]]
    assert tm.paths(3, 3, 8) == {"second_super_row": False, "partial_super_row": True, "uneven_runs": True}
    assert tm.paths(16, 1, 8) == {"second_super_row": True, "partial_super_row": False, "uneven_runs": False}


def test_gm_rule_falls_back_to_8_outside_1_to_64():
    assert [tm.gm_rule(v) for v in (0, 65, -1, 1, 2, 64, 8)] == [8, 8, 8, 1, 2, 64, 8]
    text = open(os.path.join(te.CSRC, "igemm_kernel.h")).read()
    assert 'env_int("MIXDQ_IGEMM_GM", 8)' in text and "return v >= 1 && v <= 64 ? v : 8;" in text


@pytest.mark.parametrize("family", tm.FAMILIES)
def test_every_family_reaches_every_path(family):
    got = tm.reached(family)
    assert all(got[p] for p in tm.REQUIRED[family]), (family, got)


def test_what_the_existing_edge_cases_reach():
    """tests/tile_edges.py stops at 3 x 3 tiles: under the default gm no case has a second super-row; under
    MIXDQ_IGEMM_GM = 1 and 2 (tests/env_switches.py) the three m-tiles are super-rows 1 + 1 + 1 and 2 + 1."""
    shapes = {(-(-c["M"] // te.tile(c["cfg"])[0]), -(-c["N"] // te.tile(c["cfg"])[1])) for c in te.all_linear()}
    assert max(s[0] for s in shapes) == 3
    assert not any(tm.paths(*s, 8)["second_super_row"] for s in shapes)
    assert any(tm.paths(*s, 1)["second_super_row"] for s in shapes)
    assert any(all(tm.paths(*s, 2).values()) for s in shapes)


def test_the_cases_are_what_the_table_says():
    assert len({tm.case_id(c) for c in tm.CASES}) == len(tm.CASES)
    listed = [f for s in tm.SITES.values() for f in s["families"]]
    assert sorted(listed) == tm.FAMILIES
    for c in tm.CASES:
        assert tm.case_tiles(c) == (c["tiles_m"], c["tiles_n"]), tm.case_id(c)
        tiles = c["tiles_m"] * c["tiles_n"]
        if c["family"].startswith("halo"):
            assert c["tiles_m"] in (9, 18) and c["H"] % c["TH"] == 0 and c["W"] % c["TW"] == 0
        elif c["family"].startswith("ln_"):
            assert tiles <= 256 and c["K"] % 128 == 0 and (c["K"] > 2048) == (c["family"] == "ln_global")
        else:
            assert c["tiles_m"] in tm.TILES_M and c["tiles_n"] in tm.TILES_N and tiles in (9, 11, 27, 33)
            assert c["M"] == c["tiles_m"] * c["BM"] - 5
    # the biggest case stays small
    assert max(c.get("M", 0) * max(c.get("N", 0), 1) for c in tm.CASES) <= 2811 * 768


def test_the_sites_are_the_census_of_the_run_formula():
    assert tm.census() == set(tm.SITES), {"without a row": tm.census() - set(tm.SITES),
                                          "rows without a site": set(tm.SITES) - tm.census()}
    for name, site in tm.SITES.items():
        text = open(os.path.join(te.CSRC, name)).read()
        assert ("gsz" in text) == bool(site["families"]), name          # the super-row walk is where the table says
    assert "constexpr int kNumXCD = 8;" in open(os.path.join(te.CSRC, "common.h")).read()


def test_a_further_copy_of_the_map_would_be_found(tmp_path):
    (tmp_path / "scratch.hip").write_text(
        "const int xcd = bid % kNumXCD, q8 = n / kNumXCD, r8 = n % kNumXCD;\n"
        "const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / kNumXCD;\n")
    (tmp_path / "renamed.h").write_text("const int x = b % kNumXCD, q = n / kNumXCD, r = n % kNumXCD;\n")
    (tmp_path / "other.h").write_text("const int cus = n / kNumXCD * kNumXCD;\n")
    assert tm.census(str(tmp_path)) == {"scratch.hip", "renamed.h"}


def test_coded_operands_name_their_tiles():
    a, w, acc = tm.coded_gemm(571, 188, 128, 64, 64)
    assert acc[0, 0] == tm.tile_code(0, 0) and acc[570, 187] == tm.tile_code(8, 2) and w.min() >= -2
    codes = {tm.tile_code(m, n) for m in range(13) for n in range(4)}
    assert len(codes) == 13 * 4 and max(codes) < 2048                       # distinct, exact in FP16
    a, w, acc = tm.coded_gemm_narrow(571, 188, 256, 64, 64)
    assert w.min() >= -2 and w.max() <= 1 and acc[570, 187] == tm.tile_code(8, 2)
    pt = np.arange(2 * 24 * 48).reshape(2, 24, 48) % 18
    x, w, acc = tm.coded_conv(2, 24, 48, 64, 156, pt, 80)
    from tests import exact_inputs as ei
    full = ei.conv_accumulate(x.transpose(0, 3, 1, 2), w.transpose(0, 3, 1, 2), 1, 1, dtype=np.int64)
    assert np.array_equal(full.transpose(0, 2, 3, 1), acc)
