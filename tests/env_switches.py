"""Every environment switch of the library and the package: one row per switch -- where it is read and how, the values
a test runs, what the alternative is, what is asserted of it, and where it is run.  tests/test_env_switches_host.py
holds the table equal to the census of the sources; tests/test_env_switches_gpu.py runs the rows that name it.

The relation asserted is the one the source comments claim for every switch: the SAME BITS as the default and as the
oracle (or the numpy restatement).  A switch on the C side that is read once per process (`static const ... =
env_int(...)`) runs in a child process started with the variable set: run_child() -- children run one after another,
each with its own timeout; a non-zero status, a signal or a timeout fails the test, nothing is retried and no later
child of that test is started (a driver walks the values of its switch in one test function and stops at the first
child that fails).  At most the parent and one child have the GPU open.  A switch read per launch
(`getenv` in the launch path) may be set in process; a Python module constant is set as the module attribute and
restored in `finally`.

`observable`: can a test tell from outside the launch which path ran?  Where it cannot (the tile order, the XCD map,
the payload's load policy), the child asserts that the variable was in its environment when the process started --
before the library's first launch -- and the result's bits are all there is to compare.

Imports without a GPU and without the built library.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mixdq_amd", "csrc")
GPU = "tests/test_env_switches_gpu.py"
EXPECT = "MIXDQ_TEST_EXPECT_ENV"          # "NAME=value;NAME=value": what a child asserts of its own environment

ONCE, PER_LAUNCH, PY, PY_IMPORT = "static once per process (C)", "getenv per launch (C)", "Python module constant", \
    "Python, at import"
KERNEL, GRID, SELECT, SEQUENCE = "another kernel", "another grid or other arguments", "another selection", \
    "another launch sequence"
SAME = "same bits as the default and as the oracle / restatement"


def row(name, site, read, values, alternative, run, observable=True, token=None, relation=SAME):
    return dict(name=name, site=site, read=read, values=values, alternative=alternative, relation=relation, run=run,
                observable=observable, token=token or name)


def new(test):
    return ("new", GPU, test)


def existing(path, function):
    return ("existing", path, function)


def not_run(reason):
    return ("not run", reason)


C_ROWS = [
    row("MIXDQ_IGEMM_GM", "igemm_kernel.h", ONCE, ("1", "2", "64"), GRID + " (the order of the tiles)",
        new("test_tile_map_super_row_sizes"), observable=False),
    row("MIXDQ_GN_STATS_UNROLL", "fused_norm.hip", ONCE, ("1", "4"), KERNEL,
        existing("tests/test_fused_gpu.py", "test_groupnorm_statistics_pixels_in_flight_same_bits")),
    row("MIXDQ_GN_SLICED", "fused_norm.hip", ONCE, ("1",), SEQUENCE,
        existing("tests/test_fused_gpu.py", "test_groupnorm_sliced_apply_pass_same_bits")),
    row("MIXDQ_GN_SILU_TAB", "fused_norm.hip", ONCE, ("1",), KERNEL,
        existing("tests/test_norm_edges_gpu.py", "test_launch_switches_groupnorm_same_bits")),
    row("MIXDQ_GN_SILU_TAB_MIN", "fused_norm.hip", ONCE, ("1", "1099511627776"), KERNEL + " (the size from which the table runs)",
        new("test_groupnorm_silu_table_threshold")),
    row("MIXDQ_LN_ROWS", "fused_norm.hip", ONCE, ("1", "2"), KERNEL + " and grid (rows per wave)",
        new("test_layernorm_rows_per_wave"), observable=False),
    row("MIXDQ_GEGLU_TAB", "fused_norm.hip", ONCE, ("1",), KERNEL,
        existing("tests/test_norm_edges_gpu.py", "test_launch_switches_geglu_table_same_bits")),
    # (the two parity cases of tests/test_fused_gpu.py with K > 1280 assert the DEFAULT rule's answer, select_id == -1,
    #  and cannot run under MIXDQ_LN_MAXK; under MIXDQ_LN_LOCAL they are left out for their wall time -- 6.7 G
    #  multiply-adds of CPU oracle each.  Long K under either switch: test_case_gemm_layernorm_long_k, K = 2560 and 5120)
    row("MIXDQ_LN_MAXK", "igemm_ln.hip", ONCE, ("5120",), SELECT, new("test_gemm_layernorm_record_forms_and_long_k")),
    row("MIXDQ_LN_LOCAL", "igemm_ln.hip", ONCE, ("0", "1"), GRID + " (the record form and the tile order)",
        new("test_gemm_layernorm_record_forms_and_long_k"), observable=False),
    row("MIXDQ_IGEMM_PERSIST_WGS", "igemm_pp.h", PER_LAUNCH, ("8", "16"), GRID,
        existing("tests/test_fused_gpu.py", "test_persistent_tile_loop_same_bits_with_several_tiles_per_workgroup")),
    row("MIXDQ_IGEMM_PERSIST", "igemm_pp.h", ONCE, ("0", "1"), SELECT,
        existing("tests/test_cabi.py", "test_persistent_form_is_a_switchable_choice_of_the_rule")),
    row("MIXDQ_IGEMM_TUNE", "igemm.hip", ONCE, ("300x256x256=35,300x320x256=42",), SELECT,
        new("test_tune_overrides")),
    # (tests/test_halo_w4_gpu.py is NOT run under these two: test_w4_halo_kernel_bit_exact asserts that
    #  mixdq_conv_halo_select answers a halo tile, which is false under either switch, and its other oracle tests force
    #  a halo tile (which the switches do not reach) or need the upsample fold, which only the halo kernel has.  The packed shapes of HALO_SHAPES in the new file -- three of its
    #  unforced shapes -- stand in for it: unforced, against the oracle, with the query answering 0)
    row("MIXDQ_HALO_CONV", "igemm.hip", ONCE + "; " + PER_LAUNCH + " in mixdq_conv_halo_select", ("0",), KERNEL,
        new("test_halo_switches")),
    row("MIXDQ_HALO_W4", "igemm.hip", ONCE, ("0",), KERNEL, new("test_halo_switches")),
    row("MIXDQ_RESCALE_COMBINE_LAUNCH", "sampler_rescale.hip", ONCE, ("1",), SEQUENCE,
        new("test_rescale_combine_launch")),
    row("MIXDQ_ATTN_XCD", "attention.hip", ONCE, ("0", "1"), GRID + " (the order of the blocks)",
        existing("tests/test_attention_gpu.py", "test_attention_xcd_map_changes_where_a_block_runs_not_what_it_computes"),
        observable=False),
    row("MIXDQ_PREFETCH_BLOCKS", "attention.hip", ONCE, ("8", "0"), GRID, new("test_prefetch_payload_switches"),
        observable=False),
    row("MIXDQ_PREFETCH_NT", "attention.hip", ONCE, ("1",), GRID + " (the payload's load policy)",
        new("test_prefetch_payload_switches"), observable=False),
    row("MIXDQ_PREFETCH_DELAY", "attention.hip", ONCE, ("2",), GRID + " (the payload's start)",
        new("test_prefetch_payload_switches"), observable=False),
    row("MIXDQ_ATTN_HD_SHORT", "attention.hip", ONCE, ("0", "1"), KERNEL,
        existing("tests/test_attention_hd_short_gpu.py", "test_short_form_switch_off_gives_the_same_bits")),
    row("MIXDQ_ATTN_SHORT", "attention.hip", ONCE, ("0",), KERNEL, new("test_attention_short_switch_off"),
        observable=False),
]

PY_ROWS = [
    row("MIXDQ_HIP_LIB", "_C.py", PY_IMPORT, (), "another library file",
        not_run("names the library to load, no path through it; the ABI check of mixdq_amd/_C.py guards it"),
        relation="none"),
    row("MIXDQ_EPILOGUE_VARIANT", "_C.py", PY, ("A", "B"), KERNEL + " (the epilogue's rounding)",
        existing("tests/test_conv_geometry_gpu.py", "epilogue_variant"), token="FLAGS",
        relation="each variant against the oracle's"),
    row("MIXDQ_F16IN", "_C.py", PY, ("0", "1"), SEQUENCE,
        existing("tests/test_f16in_gpu.py", "test_modules_take_the_one_launch_path_and_keep_their_bits")),
    row("MIXDQ_LN_FUSE", "_C.py", PY, ("0",), SEQUENCE, new("test_unet_switches_same_bits")),
    row("MIXDQ_CONTROL_ADD", "unet.py", PY, ("0",), SEQUENCE,
        existing("tests/test_control_gpu.py", "test_the_torch_form_of_the_adds_gives_the_same_bits")),
    row("MIXDQ_SHORTCUT_STREAM", "unet.py", PY, ("1",), SEQUENCE + " (a second stream)",
        new("test_unet_shortcut_side_stream_eager_only"),
        relation=SAME + "; eager only: a second stream inside a captured graph makes parallel branches, which this "
                        "suite does not add to graph replay"),
    row("MIXDQ_GN_RAW", "unet.py", PY, ("0",), SEQUENCE, new("test_unet_switches_same_bits")),
    row("MIXDQ_CROSS_FUSE_MAX_ROWS", "unet.py", PY, ("0",), SEQUENCE, new("test_unet_switches_same_bits")),
    row("MIXDQ_LN_CHAIN", "unet.py", PY, ("1",), SEQUENCE, existing("tests/test_unet_full_gpu.py", "_check_graph"),
        token="LN_CHAIN"),
    row("MIXDQ_PREFETCH", "unet.py", PY, ("0",), GRID + " (no payload workgroups)", new("test_unet_switches_same_bits")),
    row("MIXDQ_WEIGHT_ARENA", "unet.py", PY, ("1",), "other addresses of every static tensor",
        new("test_unet_weight_arena_same_bits")),
    row("MIXDQ_PREFETCH_MAX_ROWS", "unet.py", PY, ("4096",), "another payload plan",
        existing("tests/test_host.py", "test_prefetch_plan_own_interval_first_bounded_look_back_and_row_limit"),
        token="PREFETCH_MAX_ROWS", relation="the plan's rules; what a payload does to results: MIXDQ_PREFETCH"),
    row("MIXDQ_PREFETCH_MB", "unet.py", PY, (), "another payload plan",
        existing("tests/test_host.py", "test_prefetch_plan_own_interval_first_bounded_look_back_and_row_limit"),
        token="PREFETCH_MB_PER_LAUNCH", relation="the plan's rules; what a payload does to results: MIXDQ_PREFETCH"),
    row("MIXDQ_PREFETCH_LEAD", "unet.py", PY, (), "another payload plan",
        existing("tests/test_host.py", "test_prefetch_plan_own_interval_first_bounded_look_back_and_row_limit"),
        token="PREFETCH_MAX_LEAD", relation="the plan's rules; what a payload does to results: MIXDQ_PREFETCH"),
    row("MIXDQ_PREFETCH_SKIP_MB", "unet.py", PY, (), "another payload plan",
        not_run("an experiment's knob of the payload planner (0: off); a payload only reads: MIXDQ_PREFETCH's row "
                "covers what any plan can do to a result"), relation="none"),
    row("MIXDQ_BOS_BUFFERS_MAX", "nn/glue.py", PY, ("2",), "allocate + copy instead of a kept buffer",
        existing("tests/test_host.py", "test_kept_bos_buffers_are_bounded_in_number_and_refilled_when_the_row_changes"),
        token="BOS_BUFFERS_MAX", relation="host logic of the kept buffers"),
]

ROWS = C_ROWS + PY_ROWS


# ------------------------------------------------------------------------------------------------ the census
C_READ = re.compile(r"\b(?:env_int64|env_int|env_flag|getenv)\(\s*\"(\w+)\"")
PY_READ = re.compile(r"environ\.get\(\s*[\"'](MIXDQ_\w+)[\"']")


def census_c(csrc=CSRC):
    """{(variable, file)} of every env_int( / env_int64( / env_flag( / getenv( of a literal name under csrc/."""
    found = set()
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            for var in C_READ.findall(open(os.path.join(csrc, name)).read()):
                found.add((var, name))
    return found


def census_py(pkg=os.path.join(ROOT, "mixdq_amd")):
    """{(variable, file relative to the package)} of every os.environ read of a MIXDQ_ name in the package."""
    found = set()
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                path = os.path.join(base, f)
                for var in PY_READ.findall(open(path).read()):
                    found.add((var, os.path.relpath(path, pkg)))
    return found


def function_text(path, function):
    """Source of a top-level function (decorators included) of a test file, or None."""
    text = open(os.path.join(ROOT, path)).read()
    m = re.search(r"^((?:@[^\n]*\n(?:[ \t]+[^\n]*\n)*)*)def " + re.escape(function) + r"\(.*?(?=^\S|\Z)", text,
                  flags=re.S | re.M)
    return m.group(0) if m else None


# ------------------------------------------------------------------------------------------------ MIXDQ_IGEMM_GM
def gm_edge_nodes():
    """Node ids of tests/test_tile_edges_gpu.py and of the FP16 tile-edge test of tests/test_f16_exact_gpu.py: every
    configuration once per form, at its case with the most m-tiles (three wherever the form has an M = 2 BM + 1 case:
    super-rows 1 + 1 + 1 under MIXDQ_IGEMM_GM=1, 2 + 1 under 2).  tests/tile_edges.py gives the conv form images of one
    or two m-tiles, the grouped form and the persistent GEGLU case two: those reach a second super-row under 1 only, or
    nothing of the map (one m-tile); the conv, grouped and GEGLU forms on 11 m-tiles are tests/test_tile_map_gpu.py's.  The whole files under the switch took three times the
    wall time of the reference child: this is the selection by configuration instead of by K edge.
    -> ({part: [node id]}, {form: {configuration: m-tiles}}); the parts (one child each) are the Linear form, the GEGLU
    form, and the rest."""
    from tests import tile_edges as te
    edges, exact = "tests/test_tile_edges_gpu.py", "tests/test_f16_exact_gpu.py"
    nodes, seen = {"linear": [], "geglu": [], "other": []}, {}

    def pick(form, cfg, cases, rows, bm, tests, ident):
        c = max(cases, key=rows)                              # (the first of the cases with the most rows)
        seen.setdefault(form, {})[cfg] = -(-rows(c) // bm)
        nodes[form if form in ("linear", "geglu") else "other"].extend(
            f"{path}::{fn}[{ident(c)}]" for path, fn in tests)

    m_of = lambda c: c["M"]
    for cfg in sorted(te.IGEMM):
        bm = te.tile(cfg)[0]
        pick("linear", cfg, te.linear_cases(cfg), m_of, bm, [(edges, "test_linear_tile_edges")], te.linear_id)
        pick("conv", cfg, te.conv_cases(cfg),
             lambda c: c["n"] * ((c["H"] + 2 * c["pad"] - c["R"]) // c["stride"] + 1)
             * ((c["W"] + 2 * c["pad"] - c["R"]) // c["stride"] + 1), bm, [(edges, "test_conv_tile_edges")], te.conv_id)
        if te.geglu_admissible(cfg):
            pick("geglu", cfg, te.geglu_cases(cfg), m_of, bm, [(edges, "test_geglu_tile_edges")], te.geglu_id)
    for form in ("f16", "residual", "geglu"):                 # configurations 70 / 71: the persistent kernel's cases
        pick("pp_" + form, 71, [c for c in te.pp_cases() if c["form"] == form], m_of, 256,
             [(edges, "test_persistent_kernel_grid_edges_equal_70_and_the_oracle")], te.pp_id)
    for cfg in sorted(te.AQ):
        pick("f16in", cfg, te.f16in_cases(cfg), m_of, te.tile(cfg, te.AQ)[0], [(edges, "test_f16in_tile_edges")],
             te.f16in_id)
    for cfg in sorted(te.F16):
        pick("f16", cfg, te.f16_cases(cfg), m_of, te.tile(cfg, te.F16)[0],
             [(edges, "test_f16_tile_edges_every_configuration_same_bits"),
              (exact, "test_linear_f16_tile_edges_every_configuration_exact")], te.f16_id)
    for cfg in sorted(te.GROUPED):
        pick("grouped", cfg, te.grouped_cases(cfg), m_of, te.tile(cfg, te.GROUPED)[0],
             [(edges, "test_grouped_tile_edges_members_equal_their_own_launches")], te.grouped_id)
    return nodes, seen


# ------------------------------------------------------------------------------------------------ children
def expect_value(env):
    return ";".join(f"{k}={v}" for k, v in sorted(env.items()))


def check_expected_env():
    """In a child: every variable the parent says it set is in this process's environment (it was there when the
    process started: nothing in the tests sets these).  Returns what was expected, {} in a parent."""
    want = dict(kv.split("=", 1) for kv in os.environ.get(EXPECT, "").split(";") if kv)
    for k, v in want.items():
        assert os.environ.get(k) == v, (k, os.environ.get(k), v)
    return want


def run_child(env, targets, selection=None, timeout=120):
    """`python -m pytest targets -m gpu -x [-k selection]` in a fresh process with `env` set.  Returns (stdout,
    seconds).  Fails the calling test on a non-zero status, a signal (negative status) or the timeout: 120 s by default,
    twenty times what a child takes -- start-up and about a hundred small cases."""
    import time
    cmd = [sys.executable, "-m", "pytest", *targets, "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"]
    if selection:
        cmd += ["-k", selection]
    full = dict(os.environ, **env)
    full[EXPECT] = expect_value(env)
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=full, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=timeout)
    except subprocess.TimeoutExpired as e:
        raise AssertionError(f"child {env} ran past {timeout} s:\n{(e.stdout or '')[-3000:]}")
    dt = time.perf_counter() - t0
    assert r.returncode == 0, (env, r.returncode, r.stdout[-3000:])
    assert " passed" in r.stdout and "failed" not in r.stdout and " error" not in r.stdout, (env, r.stdout[-3000:])
    print(f"child {expect_value(env) or '(default)'}: {dt:.1f} s, {r.stdout.strip().splitlines()[-1]}")
    return r.stdout, dt
