"""The environment switches of tests/env_switches.py on the GPU.

Three kinds of test live here:
  * drivers (test_<what>_...: one per row of the table that names this file): they start child processes with a
    switch set (tests/env_switches.py run_child), one value and part after the other inside one test, and run nothing
    on the GPU themselves;
  * cases (test_case_...): what the children select, together with existing tests of other files.  They also run in
    the parent, where they check the DEFAULT path; they read the environment only to know which path to expect;
  * the Python-side switches, in process on a tiny quantized UNet.

Every comparison is bit for bit."""
import os

import numpy as np
import pytest
import torch

from tests import detdata as dd
from tests import env_switches as es
from tests import rescale_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ME = es.GPU


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scal(v):
    return torch.tensor(float(v), dtype=torch.float32, device=DEV)


def bits(a):
    a = a.detach().cpu().contiguous().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {g.size} elements differ"


def _flag(name, on_by_default):
    """csrc/common.h env_flag."""
    e = os.environ.get(name)
    return not (e and e[0] == "0") if on_by_default else bool(e and e[0] == "1")


def _child(env, targets, selection=None, timeout=120):
    """One child; its wall time is printed by run_child (pytest -s, or the captured output of a failure).  A driver
    calls this once per value and part, in a row: the first child that fails ends the driver."""
    assert es.EXPECT not in os.environ, "a driver was selected inside a child"
    es.run_child(env, targets, selection, timeout)


# ================================================================================================ what children check
def test_case_environment_is_what_the_parent_set():
    """First in every child: the switches the parent names are in this process's environment (they were when it
    started, before the library was loaded: no test sets them)."""
    es.check_expected_env()


# ---------------------------------------------------------------------------------------------- MIXDQ_IGEMM_GM
ENV_NODE = f"{ME}::test_case_environment_is_what_the_parent_set"
# the index-coded cases on 11 m-tiles (M = 699, 1403, 2811 on 64-, 128- and 256-row tiles: super-rows of 1 or 2 and, for
# 2, a partial last one); every case of the file took longer than the reference child, and the halo tiles' map has its
# super-row size built in: the switch does not reach it
GM_MAP_CODED = ("environment_is_what or ((past_one_super_row or both_record_forms) and coded and "
                "(_m699_ or _m1403_ or _m2811_))")


def test_tile_map_super_row_sizes():
    """MIXDQ_IGEMM_GM = 1 and 2 (read once per process; not observable from outside a launch), four children each:
    tests/test_tile_edges_gpu.py and the FP16 tile-edge test of tests/test_f16_exact_gpu.py, every configuration once
    per form at its case with the most m-tiles (tests/env_switches.py gm_edge_nodes: three, super-rows of 1 + 1 + 1 and
    2 + 1, for all forms but conv, grouped and the persistent GEGLU case) -- the Linear form, the GEGLU form, the other
    forms --, then the index-coded cases of tests/test_tile_map_gpu.py on 11 m-tiles.  MIXDQ_IGEMM_GM = 64, one
    super-row everywhere: those map cases again."""
    parts = es.gm_edge_nodes()[0]
    for gm in ("1", "2"):
        for part in ("linear", "geglu", "other"):
            _child({"MIXDQ_IGEMM_GM": gm}, [ENV_NODE] + parts[part])
        _child({"MIXDQ_IGEMM_GM": gm}, [ME, "tests/test_tile_map_gpu.py"], GM_MAP_CODED)
    _child({"MIXDQ_IGEMM_GM": "64"}, [ME, "tests/test_tile_map_gpu.py"], GM_MAP_CODED)


# ---------------------------------------------------------------------------------- MIXDQ_RESCALE_COMBINE_LAUNCH
# images: the factor launch's second 64-lane block (65, 130) and its masked lanes (1, 65, 130); n_image: one chunk on the
# element-by-element path, two chunks, four chunks with a partial last one
RESCALE_IMAGES, RESCALE_N = (1, 64, 65, 130), (252, 2072, 6400)


@pytest.mark.parametrize("rows", [2, 3])
@pytest.mark.parametrize("n_image", RESCALE_N)
@pytest.mark.parametrize("images", RESCALE_IMAGES)
def test_case_rescale_factor_slots(C, images, n_image, rows):
    """One rescaled step against tests/rescale_ref.py, and the r[b] slots behind the chunk statistics of the
    workspace: the restatement's factors where MIXDQ_RESCALE_COMBINE_LAUNCH=1 ran the factor launch, the caller's
    fill where the step combined the chunks itself -- the one switch whose path shows from outside.  Past the
    table nothing is written in either mode."""
    from tests import test_rescale_gpu as TR
    combine = _flag("MIXDQ_RESCALE_COMBINE_LAUNCH", False)
    c = TR._Case(rows, n_image, images, "plain", 0, seed=41 * rows + n_image + images).device(C)
    chunks = (n_image + RR.CHUNK - 1) // RR.CHUNK
    assert c.ws.numel() == images * (4 * chunks + 1) and bool(torch.isnan(c.ws).all())
    e = c.eps()
    got_in = c.launch(C, e)
    want_in, r = c.reference(0, c.blocks(e))
    c.check(got_in, want_in, f"images {images} n_image {n_image} rows {rows}")
    assert r.shape == (images,) and r.dtype == np.float32 and np.isfinite(r).all()
    assert len(np.unique(r)) >= min(images, 3)                    # (three kinds of image: different factors)
    stats, slots = c.ws[:4 * images * chunks], c.ws[4 * images * chunks:]
    assert bool(torch.isfinite(stats).all()), "a chunk's statistics were not written"
    if combine:
        same(slots, r, "the factor launch's r[b]")
    else:
        assert bool(torch.isnan(slots).all()), "the default step wrote the factor slots"
    # past the table: the statistics, the factors and the state stay as they are
    c.ws.fill_(float("nan"))
    c.step_d.fill_(3)
    x_before = c.x_d.clone()
    assert (c.launch(C, e) == TR.PAD).all()
    assert bool(torch.isnan(c.ws).all()) and torch.equal(c.x_d, x_before)


def test_rescale_combine_launch():
    """MIXDQ_RESCALE_COMBINE_LAUNCH=1: sampler_rescale_factor_kernel, which no other test runs on a GPU."""
    _child({"MIXDQ_RESCALE_COMBINE_LAUNCH": "1"}, [ME, "tests/test_rescale_gpu.py"],
           "environment_is_what or rescale_factor_slots or rescaled_step_equals_the_restatement or "
           "past_the_table or every_image_of_a_batch")


# ------------------------------------------------------------------------------------------------ MIXDQ_LN_ROWS
def test_layernorm_rows_per_wave():
    """MIXDQ_LN_ROWS = 1 and 2: the LayerNorm cases of tests/norm_edges.py -- two rows per wave at M = 1, 3, 5 (the
    absent second row), one row per wave at M = 8193."""
    for rows in ("1", "2"):
        _child({"MIXDQ_LN_ROWS": rows}, [ME, "tests/test_norm_edges_gpu.py"],
               "environment_is_what or test_layernorm_edge")


# ---------------------------------------------------------------------------------------- MIXDQ_GN_SILU_TAB_MIN
def test_groupnorm_silu_table_threshold():
    """MIXDQ_GN_SILU_TAB_MIN (a 64-bit value: the element count from which the GroupNorm apply pass takes SiLU from
    its table): 1 -- the table wherever the launch form allows it: the SiLU cases of tests/norm_edges.py below the
    default of 2 Mi elements -- and 2^40 -- never by size: the SiLU cases at and above the default (128 channels x 16384
    pixels is exactly 2 Mi; 512 x 8192; 3 x 320 x 4224).  The cases without SiLU never take the table and stay out, as
    do the second-epsilon copies: all 52 took longer than the reference child."""
    for v, cases in (("1", "silu and not vae and not hw4224"),
                     ("1099511627776", "silu and (vae_c128_hw16384 or vae_c512 or hw4224) and not eps")):
        _child({"MIXDQ_GN_SILU_TAB_MIN": v}, [ME, "tests/test_norm_edges_gpu.py"],
               f"environment_is_what or (test_groupnorm_edge and {cases})")


# ----------------------------------------------------------------------------------------------- MIXDQ_ATTN_SHORT
def test_attention_short_switch_off():
    """MIXDQ_ATTN_SHORT=0: the tkv <= 128 cases of test_attention_vs_oracle and its quantized-output sibling, the
    short-key identity test, and the causal tests (which keep the short kernel by rule)."""
    from tests import test_attention_gpu as TA
    ids = [f"b{c[0]}_q{c[1]}_k{c[2]}_c{c[3]}_{'f' if c[4] else 's'}_w{c[5]}" for c in TA.SMALL if c[2] <= 128]
    assert len(ids) == len(set(ids)) >= 10
    nodes = [ENV_NODE]
    for fn in ("test_attention_vs_oracle", "test_attention_quantized_output_is_quantize_of_fp16_output"):
        nodes += [f"tests/test_attention_gpu.py::{fn}[{i}]" for i in ids]
    nodes += ["tests/test_attention_gpu.py::test_attention_short_key_kernel_is_bit_identical_to_the_pipelined_one",
              "tests/test_attention_causal_gpu.py"]
    _child({"MIXDQ_ATTN_SHORT": "0"}, nodes)


# ---------------------------------------------------------------------------- MIXDQ_LN_LOCAL, MIXDQ_LN_MAXK
@pytest.mark.parametrize("M,N,K", [(250, 640, 2560), (300, 1280, 5120)])
def test_case_gemm_layernorm_long_k(C, oracle, M, N, K):
    """Past the default bound of the select rule (K <= 1280), inside MIXDQ_LN_MAXK=5120; tile 45 either way.  Unforced
    where the rule takes it, else on the tile it would take; the oracle's chain; the sticky error word.  (The long-K
    cases of either record form under MIXDQ_LN_LOCAL: the parity cases of tests/test_fused_gpu.py with K > 1280 stay
    out of the children.)"""
    max_k = int(os.environ.get("MIXDQ_LN_MAXK", "1280"))
    sel = C._lib.mixdq_qlinear_ln_select_id(M, N, K)
    assert sel == (45 if K <= max_k else -1), (sel, max_k)
    assert C.qlinear_ln_supported(M, N, K) == (K <= max_k)
    a, w = dd.int8(2101, (M, K)), dd.int8(2102, (N, K))
    b0, sc = dd.f32(2103, (N,), -500, 500), dd.f32(2104, (N,), 2e-5, 6e-5)
    bs, r = dd.f16(2105, (N,), -1, 1), dd.normal_f16(2106, (M, N), 1.5)
    gamma = (dd.normal_f16(2107, (N,), 0.3).astype(np.float32) + 1).astype(np.float16)
    beta = dd.normal_f16(2108, (N,), 0.2)
    qp = [(float(np.float32(1) / np.float32(0.02)), -7.0), (float(np.float32(1) / np.float32(0.03)), 4.0)]
    ws = C.qlinear_ln_workspace(M, N, DEV)
    y, outs, h = C.qlinear_ln(t(a), t(w), t(sc), t(b0), t(bs), t(r), t(gamma), t(beta), 1e-5,
                              [(scal(x), scal(z)) for x, z in qp], ws, want_f16=True, _cfg=0 if sel > 0 else 45)
    assert C.qlinear_ln_status(ws) == 0
    v = C.FLAGS & 1
    y_ref = oracle.add_f16(oracle.qlinear(a, w, b0, sc, bs, v), r)
    o_ref, h_ref = oracle.layernorm_quantize(y_ref, gamma, beta, 1e-5, qp, v)
    same(y, y_ref, "rows")
    same(h, h_ref, "LayerNorm copy")
    for got, want in zip(outs, o_ref):
        same(got, want, "quantized")


LN_MAP = ("environment_is_what or gemm_layernorm_long_k or (both_record_forms and coded) or "
          "test_qlinear_ln_narrow_widths")
# tests/test_fused_gpu.py LN_GEMM_CASES: the 128-row tile, a ragged last row tile, the FP16 copy alone (the whole list
# took twice the reference child's wall time; long K under either record form is the (250, 640, 2560) case above)
LN_PARITY = ["2048-1280-1280-True-True-1-True-44", "1000-1280-1280-True-True-2-False-56",
             "77-640-640-True-True-0-True-56"]


def test_gemm_layernorm_record_forms_and_long_k():
    """MIXDQ_LN_LOCAL = 0 and 1 force either record form on every GEMM + LayerNorm launch; MIXDQ_LN_MAXK=5120 lets
    the select rule take long K.  Two children each.  The first: the index-coded launches of tests/test_tile_map_gpu.py,
    the narrow widths of tests/test_norm_edges_gpu.py and the K = 2560 and 5120 cases above, each reading the
    workspace's sticky error word after its launch.  The second: three GEMM + LayerNorm parity cases of
    tests/test_fused_gpu.py (they read the workspace's epoch and departure words, not the error word).  That test's
    two cases with K > 1280 assert the default rule's answer for them and cannot run under MIXDQ_LN_MAXK; under
    MIXDQ_LN_LOCAL they are left out for their wall time (tests/env_switches.py)."""
    for env in ({"MIXDQ_LN_LOCAL": "0"}, {"MIXDQ_LN_LOCAL": "1"}, {"MIXDQ_LN_MAXK": "5120"}):
        _child(env, [ME, "tests/test_tile_map_gpu.py", "tests/test_norm_edges_gpu.py"], LN_MAP)
        _child(env, [ENV_NODE] + [f"tests/test_fused_gpu.py::test_qlinear_ln_equals_gemm_then_layernorm_quantize[{i}]"
                                  for i in LN_PARITY])


# ------------------------------------------------------------------------------ MIXDQ_HALO_CONV, MIXDQ_HALO_W4
HALO_SHAPES = [(2, 16, 16, 64, 80, False), (1, 24, 48, 256, 160, False), (2, 16, 16, 64, 80, True),
               (1, 24, 48, 256, 160, True), (1, 16, 32, 320, 168, True)]       # n, H, W, C, K, packed W4


@pytest.mark.parametrize("shape", HALO_SHAPES, ids=[f"n{s[0]}_{s[1]}x{s[2]}_c{s[3]}_k{s[4]}_{'w4' if s[5] else 'w8'}"
                                                     for s in HALO_SHAPES])
def test_case_halo_range_unforced_vs_oracle(C, oracle, shape):
    """3x3 / stride 1 / pad 1 convs inside the halo kernel's range, unforced: the oracle's bits whichever family runs
    them, and mixdq_conv_halo_select says which: a halo tile by default, none under MIXDQ_HALO_CONV=0, none for packed
    weights under MIXDQ_HALO_W4=0."""
    from mixdq_amd.nn.utils import pack_w4
    n, H, W, Cin, K, w4 = shape
    halo_on = _flag("MIXDQ_HALO_CONV", True)
    w4_on = halo_on and _flag("MIXDQ_HALO_W4", True)
    assert (C.conv_halo_select(n, H, W, Cin, K, 3, 3, 1, 1) != 0) == halo_on
    assert (C.conv_halo_select(n, H, W, Cin, K, 3, 3, 1, 1, w4=True) != 0) == w4_on
    x = dd.int8(2201, (n, H, W, Cin))
    q = dd.int8(2202, (K, 3, 3, Cin), *((-8, 8) if w4 else (-128, 128)))
    sc, bias, zp = dd.f32(2203, (K,), 1e-4, 6e-4), dd.f16(2204, (K,), -1, 1), -11.0
    wsum = q.astype(np.float32).sum(axis=3, dtype=np.float32)
    if w4:
        packed = pack_w4(torch.from_numpy(q))
        assert np.array_equal(oracle.unpack_w4(packed.numpy()), q)
        win = packed.to(DEV).permute(0, 3, 1, 2)
    else:
        win = t(q).permute(0, 3, 1, 2)
    got = C.qconv2d_w8_a8_ohalf(t(x).permute(0, 3, 1, 2), win, t(sc), scal(1), scal(zp), t(sc),
                                t(wsum.reshape(K, 1, 3, 3)), None, t(bias), 1, 1, _w4=w4)
    want = oracle.qconv2d(x, q, sc, wsum, zp, None, bias, 1, 1, C.FLAGS & 1)
    same(got.permute(0, 2, 3, 1), want, f"conv {shape}")


def test_halo_switches():
    """MIXDQ_HALO_CONV=0 and MIXDQ_HALO_W4=0: the halo-range convs above and the 3x3 cases of
    tests/test_conv_geometry_gpu.py on the implicit-GEMM family.  tests/test_halo_w4_gpu.py cannot run under either
    switch (it asserts that the query answers a halo tile, forces tiles, or needs the upsample fold): the packed shapes
    above, three of its unforced ones, stand in for it."""
    for env in ({"MIXDQ_HALO_CONV": "0"}, {"MIXDQ_HALO_W4": "0"}):
        _child(env, [ME, "tests/test_conv_geometry_gpu.py"],
               "environment_is_what or halo_range_unforced or (geometry and 3x3_s1_p1 and (w8a8 or w4))")


# --------------------------------------------------------------------------------------------- MIXDQ_IGEMM_TUNE
TUNE = "300x256x256=35,300x320x256=42"


def test_case_tune_overrides(C, oracle):
    """Two entries: 300 x 256 x 256 -> 35 is admissible everywhere; 300 x 320 x 256 -> 42 (BN = 80) applies to the
    plain and the packed Linear and must be ignored by GEMM + GEGLU (whole 32-column groups).  The queries answer the
    override or the rule's own choice (41 and 4), and the unforced forward gives the oracle's bits either way."""
    tuned = os.environ.get("MIXDQ_IGEMM_TUNE") == TUNE
    assert tuned or "MIXDQ_IGEMM_TUNE" not in os.environ
    assert C.igemm_select_id(300, 256, 256, 256) == (35 if tuned else 41)
    assert C.igemm_select_id(300, 256, 256, 256, geglu=True) == (35 if tuned else 41)
    assert C.igemm_select_id(300, 320, 256, 256) == (42 if tuned else 4)
    assert C.igemm_select_id(300, 320, 256, 256, w4=True) == (42 if tuned else 4)
    assert C.igemm_select_id(300, 320, 256, 256, geglu=True) == 4
    assert C.igemm_select_id(300, 640, 256, 256) == 41
    v = C.FLAGS & 1
    for N in (256, 320):
        a, w = dd.int8(2301, (300, 256)), dd.int8(2302 + N, (N, 256))
        b0, sc, bias = dd.f32(2303, (N,), -300, 300), dd.f32(2304, (N,), 2e-4, 9e-4), dd.normal_f16(2305, (N,), 0.5)
        y = C.qlinear_w8_a8_ohalf(t(a), t(w), t(sc), scal(1), scal(0), t(b0), t(sc), t(b0), t(bias))
        y_ref = oracle.qlinear(a, w, b0, sc, bias, v)
        same(y, y_ref, f"linear N = {N}")
        s_inv, zp = float(np.float32(1) / np.float32(0.02)), -60.0
        perm = C.geglu_row_order(N // 2, DEV)
        g = C.qlinear_geglu(t(a), t(w)[perm].contiguous(), t(sc)[perm].contiguous(), t(b0)[perm].contiguous(),
                            t(bias)[perm].contiguous(), scal(s_inv), scal(zp))
        same(g, oracle.geglu_quantize(y_ref, s_inv, zp, v)[0], f"geglu N = {N}")


def test_tune_overrides():
    """MIXDQ_IGEMM_TUNE (parsed once per process)."""
    _child({"MIXDQ_IGEMM_TUNE": TUNE}, [ME], "environment_is_what or case_tune_overrides")


# ------------------------------------------------------------------------------------------ MIXDQ_PREFETCH_*
def test_prefetch_payload_switches():
    """MIXDQ_PREFETCH_BLOCKS=8 with MIXDQ_PREFETCH_NT=1 and MIXDQ_PREFETCH_DELAY=2, and MIXDQ_PREFETCH_BLOCKS=0 (no
    payload workgroups): the attention result with a payload is the plain launch's."""
    for env in ({"MIXDQ_PREFETCH_BLOCKS": "8", "MIXDQ_PREFETCH_NT": "1", "MIXDQ_PREFETCH_DELAY": "2"},
                {"MIXDQ_PREFETCH_BLOCKS": "0"}):
        _child(env, [ME, "tests/test_attention_gpu.py"], "environment_is_what or prefetch_payload_changes_nothing")


# ================================================================================================ Python-side switches
class LibCalls:
    """Stands in for mixdq_amd._C._lib: every C entry point called through it is noted with the stream it was
    called on -- the launch sequence of a forward."""

    def __init__(self, lib):
        self.__dict__["lib"], self.__dict__["calls"] = lib, []

    def __getattr__(self, name):
        fn = getattr(self.__dict__["lib"], name)
        calls = self.__dict__["calls"]

        def call(*a, **k):
            calls.append((name, int(torch.cuda.current_stream().cuda_stream)))
            return fn(*a, **k)
        return call

    def __setattr__(self, name, value):
        setattr(self.__dict__["lib"], name, value)


def _sequence(C, unet, inp):
    """(output, [entry point names], {streams}) of one eager forward."""
    real = C._lib
    spy = LibCalls(real)
    C._lib = spy
    try:
        with torch.no_grad():
            out = unet(**inp)[0].clone()
        torch.cuda.synchronize()
    finally:
        C._lib = real
    calls = spy.__dict__["calls"]
    return out, [c[0] for c in calls], {c[1] for c in calls}


def _warm(unet, inp):
    """A shape's first fused forward traces the weight order the prefetch plan is built from: payloads ride from the
    second on."""
    with torch.no_grad():
        unet(**inp)
    torch.cuda.synchronize()


def _slice(inp, lo, hi):
    return dict(sample=inp["sample"][lo:hi].contiguous(), timestep=inp["timestep"],
                encoder_hidden_states=inp["encoder_hidden_states"][lo:hi].contiguous(),
                added_cond_kwargs={k: v[lo:hi].contiguous() for k, v in inp["added_cond_kwargs"].items()})


def _build_tiny(C):
    """The tiny quantized UNet of tests/test_unet_gpu.py with 64-wide heads and 320 channels at its deepest level (so
    that ff.net.2 -> the next block's norm1 is inside the GEMM + LayerNorm launch's range), fused; batch 2 and batch 1
    inputs; per batch the default fused output -- checked against the de-fused reference -- and its launch sequence."""
    import mixdq_amd.unet as U
    from tests.test_unet_gpu import TINY64, _tiny_quantized_gpu
    unet, inp2, _ = _tiny_quantized_gpu(B=2, L=32, cfg=dict(TINY64, block_out_channels=(64, 128, 320)))
    unet.set_fused(True)
    inputs = {2: inp2, 1: _slice(inp2, 0, 1)}
    base = {}
    for B, inp in inputs.items():
        _warm(unet, inp)
        out, seq, streams = _sequence(C, unet, inp)
        with torch.no_grad(), U.defused():
            ref = unet(**inp)[0].clone()
        assert bool(torch.isfinite(out).all()) and len(streams) == 1
        assert torch.equal(out, ref), f"batch {B}: the default fused forward != the de-fused reference"
        base[B] = (out, seq)
    return unet, inputs, base


@pytest.fixture(scope="module")
def tiny(C):
    """One network for the switches that leave it as it was (module attributes, restored after each test)."""
    unet, inputs, base = _build_tiny(C)
    yield unet, inputs, base
    del unet
    torch.cuda.empty_cache()


def _graph_outputs(unet, inputs):
    """The forward captured and replayed (hip_graph_opt) at both batch sizes; the eager forward is put back."""
    from mixdq_amd.quantize_sdxl import hip_graph_opt
    eager = unet.forward
    hip_graph_opt(unet)
    try:
        with torch.no_grad():
            return {B: (unet(**inp)[0].clone(), unet(**inp)[0].clone()) for B, inp in inputs.items()}
    finally:
        unet.forward = eager


def _count(seq, name):
    return sum(1 for s in seq if s == name)


# name -> (module attribute path, value, baseline attributes, what of the launch sequence must change)
def _switch_cases():
    return {
        "MIXDQ_GN_RAW": ("U.GN_RAW_OUTPUTS", False, {},
                         lambda d, s: _count(s, "mixdq_quantize_f16_i8") > _count(d, "mixdq_quantize_f16_i8")),
        "MIXDQ_CROSS_FUSE_MAX_ROWS": ("U.CROSS_FUSE_MAX_ROWS", 0, {},
                                      lambda d, s: _count(d, "mixdq_qlinear_w8a8_attn") > 0
                                      and _count(s, "mixdq_qlinear_w8a8_attn") == 0),
        "MIXDQ_PREFETCH": ("U.PREFETCH", False, {},
                           lambda d, s: _count(d, "mixdq_attention_f16_prefetch") > 0
                           and _count(s, "mixdq_attention_f16_prefetch") == 0),
        "MIXDQ_LN_FUSE": ("C.LN_FUSE", False, {"U.LN_CHAIN": True},
                          lambda d, s: _count(d, "mixdq_qlinear_w8a8_ln") > 0 and _count(s, "mixdq_qlinear_w8a8_ln") == 0),
    }


class _Attrs:
    """Module attributes set for a block and restored after it."""

    def __init__(self, C, values):
        import mixdq_amd.unet as U
        self.mods, self.values, self.saved = {"U": U, "C": C}, values, {}

    def __enter__(self):
        for path, v in self.values.items():
            m, a = path.split(".")
            self.saved[path] = getattr(self.mods[m], a)
            setattr(self.mods[m], a, v)
        return self

    def __exit__(self, *exc):
        for path, v in self.saved.items():
            m, a = path.split(".")
            setattr(self.mods[m], a, v)
        return False


@pytest.mark.parametrize("name", ["MIXDQ_GN_RAW", "MIXDQ_CROSS_FUSE_MAX_ROWS", "MIXDQ_PREFETCH", "MIXDQ_LN_FUSE"])
def test_unet_switches_same_bits(C, tiny, name):
    """The module constants behind MIXDQ_GN_RAW=0, MIXDQ_CROSS_FUSE_MAX_ROWS=0, MIXDQ_PREFETCH=0 and MIXDQ_LN_FUSE=0 (on
    top of the LayerNorm chain, which is what reads it): the fused forward at batch 1 and 2, eager and replayed from a
    captured graph, gives the bits of the default fused forward and of the de-fused reference -- and the launch sequence
    (the C entry points called) really is another one."""
    unet, inputs, base = tiny
    path, value, baseline, changed = _switch_cases()[name]
    with _Attrs(C, baseline):
        default = {B: _sequence(C, unet, inp) for B, inp in inputs.items()}
        with _Attrs(C, {path: value}):
            switched = {B: _sequence(C, unet, inp) for B, inp in inputs.items()}
            graphs = _graph_outputs(unet, inputs)
    for B in inputs:
        assert torch.equal(default[B][0], base[B][0]), f"batch {B}: baseline {baseline} != default fused forward"
        assert torch.equal(switched[B][0], base[B][0]), f"batch {B}: {name} changed the result"
        assert switched[B][1] != default[B][1] and changed(default[B][1], switched[B][1]), \
            (f"batch {B}: {name} did not change the launch sequence as expected",
             sorted(set(default[B][1]) ^ set(switched[B][1])), len(default[B][1]), len(switched[B][1]))
        g1, g2 = graphs[B]
        assert torch.equal(g1, base[B][0]) and torch.equal(g2, base[B][0]), f"batch {B}: {name} under graph replay"


def test_unet_shortcut_side_stream_eager_only(C, tiny):
    """MIXDQ_SHORTCUT_STREAM=1 (SHORTCUT_SIDE_STREAM): the 1x1 shortcut convs beside norm1 / conv1 / norm2 on a side
    stream.  Eager only: inside a captured graph a second stream makes parallel branches, which this suite does not
    add to graph replay."""
    unet, inputs, base = tiny
    with _Attrs(C, {"U.SHORTCUT_SIDE_STREAM": True}):
        got = {B: _sequence(C, unet, inp) for B, inp in inputs.items()}
    for B in inputs:
        out, seq, streams = got[B]
        assert torch.equal(out, base[B][0]), f"batch {B}: the side stream changed the result"
        assert len(streams) == 2, "no launch went to a second stream"


def test_unet_weight_arena_same_bits(C):
    """MIXDQ_WEIGHT_ARENA=1 (WEIGHT_ARENA, read by prepare_fused_): every static tensor of the converted network in one
    allocation.  On a network of its own -- the arena re-homes its tensors for good: the fused forward at batch 1 and 2,
    eager and replayed from a captured graph, gives the bits it gave before (== the de-fused reference) through the
    same launches, on other addresses."""
    unet, inputs, base = _build_tiny(C)
    assert "_arena" not in unet.__dict__
    before = {id(b): b.data_ptr() for b in unet.buffers() if b.is_cuda}
    with _Attrs(C, {"U.WEIGHT_ARENA": True}):
        unet.prepare_fused_()
    assert unet.__dict__.get("_arena") is not None, "prepare_fused_ did not read WEIGHT_ARENA"
    moved = sum(1 for b in unet.buffers() if b.is_cuda and before.get(id(b), b.data_ptr()) != b.data_ptr())
    assert moved > 0, "no tensor moved into the arena"
    for B, inp in inputs.items():
        _warm(unet, inp)                                               # (prepare_fused_ dropped the prefetch plans)
        out, seq, _ = _sequence(C, unet, inp)
        assert torch.equal(out, base[B][0]), f"batch {B}: arena-backed forward != default"
        assert seq == base[B][1]                                      # the same launches, on other addresses
    for B, (g1, g2) in _graph_outputs(unet, inputs).items():
        assert torch.equal(g1, base[B][0]) and torch.equal(g2, base[B][0]), f"batch {B}: graph replay"
    del unet
    torch.cuda.empty_cache()
