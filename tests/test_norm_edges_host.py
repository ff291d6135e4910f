"""The edge cases of tests/test_norm_edges_gpu.py reach every class of the producer launches' geometry (no GPU).
The classes are restated here as assertions over the generator's derived fields; the generator's restatement of the
launch geometry is held against the library wherever the library answers without a GPU; and every case, run through
the oracle alone, lies within the float64 bound the GPU file asserts (the inputs do not make the reference itself
break the bound)."""
import numpy as np
import pytest

from tests import norm_edges as ne

GN = ne.gn_cases()
LN = ne.ln_cases()
GEGLU = ne.geglu_cases()


def by(C, G=None):
    return [c for c in GN if c["C"] == C and (G is None or c["G"] == G) and c["C1"] == c["C"]]


def test_groupnorm_cases_reach_every_chunk_count_and_finalize_path():
    g64 = {c["HW"]: c["geom"] for c in by(64, 8)}
    assert all(g["PP"] == 32 and g["threads"] == 256 for g in g64.values())
    assert {1, 31, 32, 33, 2048, 2080, 4128, 16384, 16385} <= set(g64)
    assert [g64[hw]["nchunk"] for hw in (2048, 2080, 4128, 16384, 16385)] == [64, 65, 129, 512, 257]
    assert g64[2048]["finalize"] == "self" and g64[2080]["finalize"] == "launch"
    # the finalize launch's 8 clamped loads per lane: 2, 3 and all 8 of them used, and lanes past nchunk at 65 / 129
    assert {g["finalize_k"] for g in g64.values() if g["finalize"] == "launch"} >= {2, 3, 5, 8}
    assert max(c["geom"]["nchunk"] for c in GN) == 512
    g = g64[16385]
    assert g["ppb"] == 2 * g["PP"] and g["last_chunk_pixels"] == 1 and g["half_apply"]
    # fewer pixels than pixel lanes, exactly PP, PP + 1
    assert g64[31]["nchunk"] == 1 and g64[32]["last_chunk_pixels"] == 32 and g64[33]["last_chunk_pixels"] == 1
    # statistics unroll: both rules, and unroll 4 with a clamped fourth load (three iterations)
    assert {c["geom"]["unroll"] for c in GN} == {2, 4}
    assert any(c["geom"]["unroll"] == 4 and c["geom"]["stats_iters"] % 4 for c in GN)
    assert any(c["geom"]["unroll"] == 2 and c["geom"]["stats_iters"] == 1 for c in GN)


def test_groupnorm_cases_reach_every_block_shape():
    for C, threads in ((320, 240), (960, 240), (1920, 240), (1280, 160)):
        gs = [c["geom"] for c in by(C, 32)]
        assert gs and all(g["threads"] == threads and not g["whole_waves"] for g in gs), C
        assert any(g["finalize"] == "self" and g["self_branch"] == "loop" for g in gs), C
    assert {5, 6, 7, 384, 390} <= {c["HW"] for c in by(320, 32)} and by(320, 32)[0]["geom"]["cg"] == 10
    g320 = {c["HW"]: c["geom"] for c in by(320, 32)}
    assert g320[384]["nchunk"] == 64 and g320[390]["nchunk"] == 65 and g320[5]["HW"] < g320[5]["PP"] == 6
    for C in (960, 1920):
        assert {1, 3, 130} <= {c["HW"] for c in by(C, 32)}
        assert any(c["geom"]["finalize"] == "launch" for c in by(C, 32))
    assert {c["geom"]["self_branch"] for c in GN} >= {"pair", "loop"}
    g2560 = {c["HW"]: c["geom"] for c in by(2560, 32)}
    assert {1, 64, 65, 513} <= set(g2560) and all(g["PP"] == 1 and g["nfull"] == 5 for g in g2560.values())
    assert g2560[64]["finalize"] == "self" and g2560[65]["finalize"] == "launch"
    g8192 = [c["geom"] for c in by(8192, 32)]
    assert {g["HW"] for g in g8192} == {1, 65} and all(g["OC"] == 1024 == g["threads"] for g in g8192)
    assert any(c["geom"]["G"] == c["geom"]["threads"] for c in by(2048, 256))
    assert any(c["geom"]["cg"] == 4 for c in by(32, 8)) and any(c["geom"]["cg"] == 12 for c in by(96, 8))
    assert {1, 3} <= {c["N"] for c in GN} and {True, False} == {c["silu"] for c in GN}
    for N in (1, 3):
        assert {True, False} == {c["silu"] for c in GN if c["N"] == N}


def test_groupnorm_cases_reach_the_apply_pass_forms():
    assert sum(c["geom"]["half_apply"] for c in GN) >= 2
    assert any(c["geom"]["half_apply"] and not c["geom"]["table"] for c in GN)
    # the table pass: by the default size rule, and wherever MIXDQ_GN_SILU_TAB=1 sends it
    walkers = [c for c in GN if c["N"] >= 3 and c["geom"]["table"] and c["geom"]["chunks_per_block"] >= 2]
    assert len(walkers) >= 2, [ne.gn_id(c) for c in walkers]
    for c in walkers:
        g = c["geom"]
        assert g["gx"] == ne.cdiv(2 * ne.NUM_CU, c["N"]) < g["nchunk_apply"]
    assert any(c["geom"]["nchunk_apply"] % c["geom"]["gx"] for c in walkers)    # some blocks walk one chunk more
    assert any(c["geom"]["nchunk_apply"] % c["geom"]["gx"] == 0 for c in walkers)
    assert any(c["geom"]["table"] and c["geom"]["half_apply"] for c in walkers)
    assert any(c["geom"]["PPa"] == 1 for c in walkers) and any(c["geom"]["PPa"] > c["geom"]["PP"] for c in walkers)
    forced = [c for c in GN if c["geom_tab"]["table"] and not c["geom"]["table"]]
    assert len(forced) >= 4 and any(not c["geom"]["whole_waves"] for c in forced)
    assert all(c["geom"]["table"] == (c["silu"] and c["geom"]["finalize"] == "launch"
                                      and c["N"] * c["HW"] * c["C"] >= ne.TAB_MIN) for c in GN)


def test_groupnorm_cases_reach_the_vae_widths():
    """mixdq_amd.vae's GroupNorms: 32 groups at C = 128, 256, 512, eps 1e-6 (and 1e-5), SiLU and plain."""
    vae = [c for c in GN if c["name"].startswith("vae_")]
    assert {c["eps"] for c in vae} == {1e-6, 1e-5} == set(ne.VAE_EPS) and all(c["eps"] == 1e-5 for c in GN if c not in vae)
    assert all(c["G"] == 32 for c in vae) and {c["C"] for c in vae} == {128, 256, 512}
    for eps in ne.VAE_EPS:
        mine = [c for c in vae if c["eps"] == eps]
        for C in (128, 256, 512):
            assert {True, False} == {c["silu"] for c in mine if c["C"] == C}, (eps, C)
        # groups of 4 channels under 32 groups: every octet straddles two groups, 32 reducing threads of 256
        cg4 = [c for c in mine if c["geom"]["cg"] == 4 and c["G"] == 32]
        assert cg4 and all(c["geom"]["threads"] == 256 and c["geom"]["OC"] == 16 for c in cg4)
        assert {70, 16384} <= {c["HW"] for c in cg4}
        # the table pass by the default size rule at cg == 4 (2 Mi elements), and 512 chunks
        assert any(c["geom"]["table"] and c["N"] * c["HW"] * c["C"] == ne.TAB_MIN for c in cg4)
        assert any(c["geom"]["nchunk"] == 512 for c in cg4)
        assert any(not c["silu"] and c["geom"]["nchunk"] == 512 and not c["geom"]["table"] for c in cg4)
        assert any(c["C"] == 512 and c["HW"] == 8192 and c["N"] * c["HW"] * c["C"] == ne.ELEMENT_CAP
                   and c["geom"]["nchunk"] == 512 for c in mine)
        assert any(c["C"] == 256 and c["geom"]["finalize"] == "launch" for c in mine)
    assert len({ne.gn_id(c) for c in GN}) == len(GN)


def test_groupnorm_two_source_splits():
    sp = [c for c in GN if c["C1"] != c["C"]]
    assert {"inside", "boundary"} == {c["split"] for c in sp}
    for c in sp:
        assert c["C1"] % 8 == 0 and 0 < c["C1"] < c["C"]
        assert (c["C1"] % c["geom"]["cg"] == 0) == (c["split"] == "boundary")
    assert any(c["geom"]["finalize"] == "launch" for c in sp) and any(c["geom"]["finalize"] == "self" for c in sp)


def test_groupnorm_restatement_agrees_with_the_library():
    import mixdq_amd._C as C
    shapes = [(c["N"], c["HW"], c["C"], c["G"]) for c in GN] + ne.GN_REFUSED
    shapes += [(2, hw, c, g) for hw in (1, 255, 256, 257, 511, 512, 513, 100000) for c, g in
               ((8, 1), (8, 2), (24, 3), (40, 10), (72, 6), (640, 32), (4096, 32), (8192, 2048))]
    for N, HW, Cc, G in shapes:
        want = C._lib.mixdq_groupnorm_workspace_bytes(N, HW, Cc, G)
        assert ne.gn_workspace_bytes(N, HW, Cc, G) == want, (N, HW, Cc, G)
        assert C.groupnorm_supported(N, HW, Cc, G) == (ne.gn_geom(N, HW, Cc, G) is not None)
    for s in ne.GN_REFUSED:
        assert ne.gn_geom(*s) is None and not C.groupnorm_supported(*s)
    assert any(ne.gn_geom(*s) is None for s in shapes[len(GN) + 3:])      # (the sweep meets further refusals)


def test_groupnorm_oracle_geometry_is_the_generators(oracle):
    """The oracle refuses exactly what the generator (and the library) refuses."""
    for N, HW, Cc, G in ne.GN_REFUSED:
        z = np.zeros((N, HW, Cc), np.float16)
        with pytest.raises(ValueError):
            oracle.groupnorm_silu_quantize(z, np.zeros(Cc, np.float16), np.zeros(Cc, np.float16), 1e-5, G, False, 1, 0)


@pytest.mark.parametrize("case", GN, ids=[ne.gn_id(c) for c in GN])
def test_groupnorm_oracle_within_the_float64_bound(oracle, case):
    x, gamma, beta, (s_inv, zp) = ne.gn_inputs(case)
    _, pre = oracle.groupnorm_silu_quantize(x, gamma, beta, case["eps"], case["G"], False, s_inv, zp)
    ok = ne.within_norm_bound(pre, ne.groupnorm64(x, gamma, beta, case["eps"], case["G"]))
    assert ok.all(), f"{(~ok).sum()} of {ok.size} outside the bound"


def test_layernorm_cases_reach_every_statistics_shape():
    gs = [c["geom"] for c in LN]
    assert {g["U"] for g in gs} == {1, 2, 4, 8, 16}
    assert {1, 3, 4, 5, 15, 127, 8, 2, 6} <= {g["per"] for g in gs}
    assert {(4, 5), (2, 5), (4, 15), (8, 15), (1, 127), (1, 1), (2, 1), (1, 3), (2, 3)} <= {(g["U"], g["per"]) for g in gs}
    assert {g["chunks_per_lane"] for g in gs} == {1, 2, 3, 4}
    for k in (1, 2, 3, 4):
        assert any(g["chunks_per_lane"] == k and g["partial_last_chunk"] for g in gs), k
    assert any(g["chunks_per_lane"] == 4 and not g["partial_last_chunk"] for g in gs)
    for C in ne.LN_WIDTHS:
        assert {1, 3, 4, 5} <= {c["M"] for c in LN if c["C"] == C}, C        # a block of 4 waves: under, at, over
    for C in (16, 320):
        two = [c["geom"] for c in LN if c["C"] == C and c["geom"]["rows_per_wave"] == 2]
        assert {g["M"] for g in two} == {8192, 8193} and any(g["odd_tail"] for g in two)
    assert {0, 1, 2, 3} == {c["nq"] for c in LN}
    assert all(ne.ln_geom(1, C) is None for C in ne.LN_REFUSED)
    assert set(ne.LN_WIDTHS) >= {16, 32, 48, 96, 160, 320, 512, 960, 1024, 1536, 1920, 2032, 2048}


@pytest.mark.parametrize("C", ne.LN_WIDTHS)
def test_layernorm_oracle_within_the_float64_bound(oracle, C):
    for M in sorted({c["M"] for c in LN if c["C"] == C}):
        x, gamma, beta = ne.ln_inputs(M, C)
        _, h = oracle.layernorm_quantize(x, gamma, beta, 1e-5, [])
        ok = ne.within_norm_bound(h, ne.layernorm64(x, gamma, beta, 1e-5))
        assert ok.all(), (M, C, int((~ok).sum()))


def test_geglu_cases_reach_the_grid_edges():
    gs = [c["geom"] for c in GEGLU]
    assert {(1, 8), (3, 24), (5, 8 * 127), (257, 40)} <= {(g["M"], g["D"]) for g in gs}
    assert all(g["odd_octets"] for g in gs)                                     # D = 8 * odd throughout
    capped = [c for c in GEGLU if c["geom"]["capped"]]
    assert capped and all(c["geom"]["pieces_per_thread"] == 2 and c["geom"]["stride_splits_rows"] for c in capped)
    # under MIXDQ_GEGLU_TAB=1: the table kernel's walk, its stride not a multiple of a row
    assert all(c["geom_tab"]["table"] and c["geom_tab"]["block"] == 1024 for c in GEGLU)
    assert any(c["geom_tab"]["capped"] and c["geom_tab"]["stride_splits_rows"] for c in GEGLU)
    assert any(c["geom"]["table"] for c in GEGLU) and any(not c["geom"]["table"] for c in GEGLU)
    assert any(c["geom_tab"]["total"] % 64 for c in GEGLU)                      # a ragged last wave


@pytest.mark.parametrize("case", GEGLU, ids=[ne.geglu_id(c) for c in GEGLU])
def test_geglu_oracle_within_the_float64_bound(oracle, case):
    h = ne.geglu_inputs(case["M"], case["D"])
    _, o = oracle.geglu_quantize(h, 20.0, -100.0)
    ok = ne.within_geglu_bound(o, h)
    assert ok.all(), int((~ok).sum())


def test_layernorm_in_gemm_cases_are_the_librarys_answer():
    import mixdq_amd._C as C
    sel = C._lib.mixdq_qlinear_ln_select_id
    cases = ne.ln_gemm_cases(sel)
    assert {c["N"] for c in cases} == set(ne.LN_GEMM_WIDTHS)
    for c in cases:
        if c["cfg"] is None:
            assert all(sel(M, c["N"], K) <= 0 for K in range(16, 2049, 16) for M in (1, 64, 256)), c
            continue
        assert sel(c["M"], c["N"], c["K"]) == c["cfg"] and c["cfg"] in ne.LN_GEMM_ROW_TILE
        assert c["K"] == 16 or all(sel(c["M"], c["N"], K) <= 0 for K in range(16, c["K"], 16))   # the smallest K
    for N in ne.LN_GEMM_WIDTHS:
        mine = [c for c in cases if c["N"] == N]
        assert mine[0]["cfg"] is None or any(c["ragged"] and c["M"] > ne.LN_GEMM_ROW_TILE[c["cfg"]] for c in mine), N
    # a column tile is one unit of the LayerNorm statistics (csrc/igemm_ln.hip select_ln): 4, 2, 1 units
    assert [ne.ln_geom(1, N)["U"] for N in ne.LN_GEMM_WIDTHS] == [4, 2, 1]
    assert all(ne.ln_geom(1, N)["per"] == 5 for N in ne.LN_GEMM_WIDTHS)
