"""The edge cases of tests/test_tile_edges_gpu.py cover every tile configuration (no GPU).  The required values
are restated here from each configuration's (BM, BN, BK, STAGES), independently of the generator, so that a
configuration added to the library -- or an edge dropped from the generator -- fails on the CPU."""
import os

import pytest

from tests import conv_geometry as cg
from tests import tile_edges as te


def kt(K, bk):
    return -(-K // bk)


def test_generator_tables_are_the_bindings_tables():
    """The generator reads the X-macro tables the library is compiled from; the Python bindings list the same ids
    and parameters (a configuration the bindings do not list is never forced by any test that iterates them)."""
    import mixdq_amd._C as C
    assert {i: v[:4] for i, v in te.IGEMM.items()} == C.IGEMM_CONFIGS
    assert {i: v[4:8] for i, v in te.IGEMM.items()} == C.IGEMM_WAVES
    assert tuple(sorted(te.F16)) == tuple(sorted(C.F16_CONFIGS))
    assert tuple(sorted(te.AQ)) == tuple(sorted(C.F16IN_CONFIGS))
    assert tuple(sorted(te.GROUPED)) == tuple(sorted(C.GROUPED_CONFIGS))
    assert tuple(sorted(i for i in te.IGEMM if not te.w2_admissible(i))) == tuple(sorted(C.W2_INADMISSIBLE))
    for table in (te.F16, te.AQ, te.GROUPED):            # the same ids name the same tiles
        for i, v in table.items():
            assert i in te.IGEMM and v[:4] == te.IGEMM[i][:4], i
    # what the LOADED library reports (mixdq_tile_config) is what the source tree says: the build matches the tree
    halo = te._xmacro(os.path.join(te.CSRC, "iconv.h"), "MIXDQ_HALO_TILES")
    assert {i: v[:3] for i, v in halo.items()} == C.HALO_TILES
    assert [r[:6] for r in C.tile_family(5)] == [(i, *v) for i, v in halo.items()]
    assert C.tile_family(4) == []              # GEMM+LayerNorm: ids 44, 45, 56 are cases of igemm_ln.hip, not a table
    for r in C.tile_family(0):             # ... and the admissibility rules restated in the generator
        assert r[:9] == (r[0], *te.IGEMM[r[0]]), r
        assert bool(r[9] & 2) == te.w2_admissible(r[0]) and bool(r[9] & 4) == te.geglu_admissible(r[0]), r
        assert bool(r[9] & 1) == cg.IGEMM_GATHER[r[0]][6], r            # the four-phase loop


@pytest.mark.parametrize("cfg", sorted(te.IGEMM))
def test_linear_cases_cover_the_edges(cfg):
    bm, bn, bk, st = te.IGEMM[cfg][:4]
    cases = te.linear_cases(cfg)
    assert all(c["cfg"] == cfg and c["N"] % 4 == 0 and c["K"] % 16 == 0 for c in cases)
    assert all(c["M"] <= 2 * bm + 1 and c["N"] <= 2 * bn + 4 and c["K"] <= (st + 1) * bk for c in cases)
    ks = {c["K"] for c in cases}
    for nk in {1, 2, max(st - 1, 1), st, st + 1}:
        assert nk * bk in ks, f"cfg {cfg}: no case with {nk} whole K-tiles"
        if nk * bk - 16 >= 16:
            assert nk * bk - 16 in ks, f"cfg {cfg}: no ragged case with {nk} K-tiles"
    assert {1, bm - 1, bm, bm + 1, 2 * bm + 1} <= {c["M"] for c in cases}, cfg
    assert {4, bn - 4, bn, bn + 4, 2 * bn + 4} <= {c["N"] for c in cases}, cfg
    assert any(c["N"] % 8 == 4 for c in cases)
    assert {True, False} == {c["bias"] for c in cases}
    assert any(c["residual"] for c in cases) and any(c["rowmap"] for c in cases)
    assert not any(c["residual"] and c["rowmap"] for c in cases)      # MIXDQ_ERR_ROWMAP_RESIDUAL
    # the widths the id admits: W4 wherever K % 32 == 0, W2 wherever K % 64 == 0 on an admissible tile -- at one
    # K-tile and at STAGES + 1 of them; the refusals are asserted on the others
    for nk in (1, st + 1):
        assert any(c["w4"] and kt(c["K"], bk) == nk for c in cases), (cfg, nk)
        assert any(c["w2"] and kt(c["K"], bk) == nk for c in cases), (cfg, nk)
    assert any(not c["w4"] for c in cases)
    assert all(c["w4"] == (c["K"] % 32 == 0) and c["w2"] == (c["K"] % 64 == 0) for c in cases)


@pytest.mark.parametrize("cfg", sorted(te.IGEMM))
def test_conv_cases_cover_the_edges(cfg):
    bm, bn, bk, st = te.IGEMM[cfg][:4]
    cases = te.conv_cases(cfg)
    assert {16, 48, 320, 960} <= {c["C"] for c in cases}
    assert {(3, 0), (3, 1), (1, 0)} <= {(c["R"], c["pad"]) for c in cases}
    assert {1, 2} <= {c["stride"] for c in cases if c["R"] == 3}
    assert any(c["C"] % 32 == 0 for c in cases) and any(c["C"] % 32 for c in cases)    # W4 and its refusal
    assert any(c["H"] % 2 and c["W"] % 2 for c in cases)
    assert all(bn < c["K"] < 2 * bn and c["K"] % 4 == 0 for c in cases)          # an N tail in the second tile
    assert any(kt(9 * c["C"], bk) <= st + 1 for c in cases if c["R"] == 3)      # a short pipeline


@pytest.mark.parametrize("cfg", sorted(te.IGEMM))
def test_geglu_cases_cover_the_edges(cfg):
    bm, bn, bk, st, wm, wn = te.IGEMM[cfg][:6]
    if not (bn % 32 == 0 and (bn // wn) % 32 == 0):
        assert not te.geglu_admissible(cfg)              # the GPU file asserts its refusal instead
        assert cfg not in {c["cfg"] for c in te.all_geglu()}
        return
    cases = te.geglu_cases(cfg)
    assert cfg in {c["cfg"] for c in te.all_geglu()}
    assert {1, 2, st} <= {kt(c["K"], bk) for c in cases}
    assert all(c["K"] % bk == 0 and c["N"] % 32 == 0 for c in cases)
    assert {1, bm - 1, bm, bm + 1, 2 * bm + 1} <= {c["M"] for c in cases}
    assert {32, bn - 32, bn, bn + 32, 2 * bn + 32} - {0} <= {c["N"] for c in cases}


def test_persistent_cases_cover_the_grid_edges():
    cases = te.pp_cases()
    ms, ns = {c["M"] for c in cases}, {c["N"] for c in cases}
    assert {255, 256, 257} <= ms and {511, 512, 513} <= ms
    assert {248, 264} <= ns and any(n % 8 == 4 for n in ns)
    assert {"f16", "residual", "geglu"} == {c["form"] for c in cases}
    assert any(c["K"] < 256 for c in cases)                       # below pp_ok: the non-persistent form
    assert all(c["form"] != "geglu" or c["N"] % 32 == 0 for c in cases)


@pytest.mark.parametrize("cfg", sorted(te.AQ))
def test_f16in_cases_cover_the_edges(cfg):
    bm, bn, bk, st = te.AQ[cfg][:4]
    ad = max(st - 1, 2)
    cases = te.f16in_cases(cfg)
    assert {1, 2, ad, ad + 1} <= {kt(c["K"], bk) for c in cases}
    assert all(c["K"] % bk == 0 for c in cases)
    assert {1, bm - 1, bm, bm + 1, 2 * bm + 1} <= {c["M"] for c in cases}
    assert {4, bn - 4, bn, bn + 4, 2 * bn + 4} <= {c["N"] for c in cases}


@pytest.mark.parametrize("cfg", sorted(te.F16))
def test_f16_cases_cover_the_edges(cfg):
    bm, bn, bk, st = te.F16[cfg][:4]                  # BK in bytes: 2 per FP16 element
    cases = te.f16_cases(cfg)
    kb = {2 * c["K"] for c in cases}
    for nk in {1, 2, max(st - 1, 1), st, st + 1}:
        assert nk * bk in kb and (nk * bk - 16 < 16 or nk * bk - 16 in kb), (cfg, nk)
    assert {1, bm - 1, bm, bm + 1, 2 * bm + 1} <= {c["M"] for c in cases}
    assert {4, bn - 4, bn, bn + 4, 2 * bn + 4} <= {c["N"] for c in cases}


@pytest.mark.parametrize("cfg", sorted(te.GROUPED))
def test_grouped_cases_cover_the_edges(cfg):
    bm, bn, bk, st = te.GROUPED[cfg][:4]
    cases = te.grouped_cases(cfg)
    assert {1, st} <= {kt(c["K"], bk) for c in cases}
    assert all({bn - 4, bn, bn + 4} <= set(c["Ns"]) for c in cases)
