"""What the library's host code LAUNCHES, recorded without a GPU: for every entry point that launches, over every
mode that selects a kernel instantiation, the returned status and the launches (kernel, grid, block, dynamic LDS),
LDS opt-ins, synchronisations and copies the call makes.  tests/dispatch_fixture.py pins the calls that return before
their first HIP call; this pins the ones that go on.

How: mixdq_amd/_obj/*.o (what mixdq_amd.build.build() leaves behind) are linked with g++ against
tests/launch_trace_runtime.cpp, a stand-in for the ~18 HIP runtime entry points the objects call, into
mixdq_amd/_obj/libmixdq_trace.so -- never against libamdhip64, and with -Bsymbolic, so the library's runtime calls bind
to the stand-in whatever else the process has loaded.  `python -m tests.launch_trace` drives that library with plain
ctypes (no torch) in a fresh process and prints {case: "status|event;event;..."}; the pointers are aligned dummies
that are never dereferenced (nothing runs), so a shape costs nothing.  Process state is part of what is recorded:
the first launch of a > 64 KiB-LDS instantiation on a device carries its opt-in, later ones do not.

tools/record_launch_trace.py writes tests/golden/launch_trace.json; tests/test_launch_trace_host.py compares.
What a trace does NOT see: kernel arguments (MIXDQ_ATTN_XCD, MIXDQ_PREFETCH_*, MIXDQ_IGEMM_GM only change those) and
anything a kernel does.
"""
import ctypes
import itertools
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace.json")
UNREACHED = os.path.join(ROOT, "tests", "golden", "launch_trace_unreached.json")
HEADER = os.path.join(ROOT, "include", "mixdq_hip.h")
RUNTIME_SRC = os.path.join(ROOT, "tests", "launch_trace_runtime.cpp")
# the objects to trace: this tree's, or those of another checkout (recording from the commit before a refactor)
OBJ = os.environ.get("MIXDQ_TRACE_OBJ") or os.path.join(ROOT, "mixdq_amd", "_obj")
TRACE_LIB = os.path.join(OBJ, "libmixdq_trace.so")

ERR_LAUNCH = 4
FLAG_UNFUSED, FLAG_W4, FLAG_UPS, FLAG_A_ROWMAP, FLAG_W2, FLAG_CAUSAL = 1, 2, 4, 8, 16, 32
ACT_GELU, ACT_QUICK_GELU = 64, 128
A4_0, A4_1, A4_2, PAD_AFTER = 1 << 16, 1 << 17, 1 << 18, 1 << 19
WBITS = ((0, "w8"), (FLAG_W4, "w4"), (FLAG_W2, "w2"))
LN_TILE_IDS = (44, 45, 56)          # mixdq_qlinear_ln_select_id's answers (include/mixdq_hip.h)

# One child per environment.  Every MIXDQ_* variable of the caller is dropped first: the knobs are read once per process.
KNOBS = {
    "default": {},
    "knobs": {"MIXDQ_GN_SLICED": "1", "MIXDQ_GN_SILU_TAB": "0", "MIXDQ_GEGLU_TAB": "1", "MIXDQ_LN_ROWS": "2",
              "MIXDQ_GN_STATS_UNROLL": "1", "MIXDQ_ATTN_SHORT": "0", "MIXDQ_ATTN_HD_SHORT": "0", "MIXDQ_IGEMM_GM": "4"},
    "knobs_tab": {"MIXDQ_GN_SILU_TAB": "1", "MIXDQ_GEGLU_TAB": "0", "MIXDQ_LN_ROWS": "1"},
}


# ------------------------------------------------------------------------------------------- the trace library
def build_trace_lib():
    """Link the stand-in runtime and the library's objects (when any of them is newer than the result) and check that
    no HIP runtime symbol is left for the dynamic linker to find elsewhere."""
    objs = sorted(os.path.join(OBJ, f) for f in os.listdir(OBJ) if f.endswith(".o"))
    assert objs, f"no objects under {OBJ}: run mixdq_amd.build.build() first"
    deps = objs + [RUNTIME_SRC]
    if not os.path.exists(TRACE_LIB) or any(os.path.getmtime(d) > os.path.getmtime(TRACE_LIB) for d in deps):
        tmp = TRACE_LIB + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-o", tmp,
                               RUNTIME_SRC] + objs)
        os.replace(tmp, TRACE_LIB)
    undefined = subprocess.run(["nm", "-D", "--undefined-only", TRACE_LIB], capture_output=True, text=True,
                               check=True).stdout.split("\n")
    left = [l.split()[-1] for l in undefined if l.strip() and re.match(r"_*hip", l.split()[-1], re.I)]
    assert not left, f"the trace library still needs {left} from a HIP runtime: add them to {RUNTIME_SRC}"
    return TRACE_LIB


def _ctype(decl):
    if "*" in decl or "mixdq_stream_t" in decl:
        return ctypes.c_void_p
    t = decl.split()[-2] if len(decl.split()) > 1 else decl
    return {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "float": ctypes.c_float, "size_t": ctypes.c_size_t}[t]


def signatures():
    """{entry point: [(argument name, ctypes type)]} of every int-returning function of include/mixdq_hip.h."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"^int\s+(mixdq_\w+)\s*\(([^;]*?)\)\s*;", text, re.M | re.S):
        args = [" ".join(a.split()) for a in m.group(2).split(",")]
        if args == ["void"]:
            continue
        out[m.group(1)] = [(re.split(r"[\s*]+", a)[-1], _ctype(a)) for a in args]
    return out


def ptr(i):
    """An aligned dummy pointer, distinct per operand and 1 TiB from the next: no two operands overlap."""
    return i << 40


class Tracer:
    def __init__(self):
        self.lib = ctypes.CDLL(build_trace_lib())
        self.lib.launch_trace_take.restype = ctypes.c_char_p
        self.lib.launch_trace_kernels.restype = ctypes.c_char_p
        self.lib.launch_trace_set_capture.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
        self.sig = signatures()
        self.kernels = sorted(self.lib.launch_trace_kernels().decode().split())
        assert len(set(self.kernels)) == len(self.kernels)
        self.index = {k: i for i, k in enumerate(self.kernels)}
        self.out = {}
        self.keep = []               # host arrays that calls point into

    def entry(self, name, **base):
        return Entry(self, name, base)

    def host(self, ctype, values):
        a = (ctype * len(values))(*values)
        self.keep.append(a)
        return ctypes.cast(a, ctypes.c_void_p).value

    def events(self):
        """The log since the last call, compact: L<kernel index>:<grid>:<block>:<lds>, A<kernel index>:<bytes>
        (the opt-in), S (a synchronisation), T / F / M <bytes> (to symbol, from symbol, plain copy)."""
        out = []
        for line in self.lib.launch_trace_take().decode().split("\n"):
            w = line.split()
            if not w:
                continue
            if w[0] == "launch":
                out.append(f"L{self.index[w[1]]}:{w[2]}:{w[3]}:{w[4]}")
            elif w[0] == "attr":
                out.append(f"A{self.index[w[1]]}:{w[2]}")
            else:
                out.append({"sync": "S", "to_symbol": "T", "from_symbol": "F", "memcpy": "M"}[w[0]] + "".join(w[1:]))
        return out


class Entry:
    """One entry point: a base call that launches, and cases as overrides of its arguments.  Pointer arguments the
    base does not name are distinct aligned dummies."""

    def __init__(self, tracer, name, base):
        self.t, self.name, self.args = tracer, name, tracer.sig[name]
        self.fn = getattr(tracer.lib, name)
        self.fn.argtypes, self.fn.restype = [c for _, c in self.args], ctypes.c_int
        names = [a for a, _ in self.args]
        assert set(base) <= set(names), (name, set(base) - set(names))
        self.base = {a: ptr(i + 1) for i, (a, c) in enumerate(self.args) if c is ctypes.c_void_p and a != "stream"}
        self.base.update(stream=None, hip_stream=None)
        self.base.update(base)
        missing = [a for a in names if a not in self.base]
        assert not missing, (name, missing)

    def case(self, label, **over):
        assert set(over) <= set(self.base), (self.name, over)
        key = f"{self.name[6:]}/{label}"
        assert key not in self.t.out, key
        a = dict(self.base, **over)
        status = self.fn(*(a[n] for n, _ in self.args))
        self.t.out[key] = "|".join([str(status), ";".join(self.t.events())])


def forced(i):
    return i << 8


def tile_ids(lib, family):
    row = (ctypes.c_int * 10)()
    n = lib.mixdq_tile_config(family, 0, row)
    ids = []
    for i in range(n):
        lib.mixdq_tile_config(family, i, row)
        ids.append(row[0])
    return ids


def flag_cases(pairs):
    """Every combination of the given (flag, name) options: [(flags, label)]; the empty combination is 'plain'."""
    out = []
    for pick in itertools.product((False, True), repeat=len(pairs)):
        f = sum(p[0] for p, on in zip(pairs, pick) if on)
        out.append((f, "_".join(p[1] for p, on in zip(pairs, pick) if on) or "plain"))
    return out


# ------------------------------------------------------------------------------------------------------ cases
def norm_entries(t):
    gn1 = t.entry("mixdq_groupnorm_silu_quantize", eps=1e-5, apply_silu=1, N=1, HW=4096, C=320, G=32, flags=0)
    gn2 = t.entry("mixdq_groupnorm_silu_quantize2", C1=320, eps=1e-5, apply_silu=1, N=1, HW=4096, C=640, G=32, flags=0)
    raw = dict(raw_scale_inv=t.host(ctypes.c_void_p, [ptr(40), ptr(41)]),
               raw_zero_point=t.host(ctypes.c_void_p, [ptr(42), ptr(43)]),
               raw_q=t.host(ctypes.c_void_p, [ptr(44), ptr(45)]))
    gn3 = t.entry("mixdq_groupnorm_silu_quantize3", C1=320, eps=1e-5, apply_silu=1, N=1, HW=4096, C=640, G=32, flags=0,
                  **raw)
    ln_arrays = dict(scale_inv=t.host(ctypes.c_void_p, [ptr(50), ptr(51), ptr(52)]),
                     zero_point=t.host(ctypes.c_void_p, [ptr(53), ptr(54), ptr(55)]),
                     out_q=t.host(ctypes.c_void_p, [ptr(56), ptr(57), ptr(58)]))
    ln = t.entry("mixdq_layernorm_quantize", eps=1e-5, M=5, C=1280, n_out=1, flags=0, **ln_arrays)
    geglu = t.entry("mixdq_geglu_quantize", M=64, D=1280, flags=0)
    return gn1, gn2, gn3, ln, geglu


# (the shapes of the three table consumers: large enough that the default rule takes the table)
GN_TAB = dict(HW=16384)
GEGLU_TAB = dict(M=1024, D=5120)


def sequences(t):
    """Process state, in the order that shows it: the three table builders under capture ids, then the opt-in per
    device.  First in the process: the tables are not built yet and no instantiation has opted in."""
    lib = t.lib
    gn1, _, _, _, geglu = norm_entries(t)
    gemm_geglu = t.entry("mixdq_qlinear_w8a8_geglu", M=1024, N=2560, K=640, flags=0)
    for entry, shape, name in ((gemm_geglu, {}, "gemm_geglu"), (gn1, GN_TAB, "gn_silu"), (geglu, GEGLU_TAB, "geglu")):
        for i, (status, cap) in enumerate(((1, 7), (1, 7), (1, 9), (0, 0), (0, 0))):
            lib.launch_trace_set_capture(status, cap)
            entry.case(f"seq_table_{name}_{i}_capture{cap}", **shape)
    lib.launch_trace_set_capture(0, 0)
    rows = t.entry("mixdq_qlinear_w8a8_rows", M=1024, N=1280, K=1280, group_rows=0, group_stride=0, group_offset=0,
                   residual_f16_or_null=None, residual_row_div=1, flags=forced(20))
    pp = t.entry("mixdq_qlinear_w8a8_rows", M=8192, N=10240, K=1280, group_rows=0, group_stride=0, group_offset=0,
                 residual_f16_or_null=None, residual_row_div=1, flags=0)
    att = t.entry("mixdq_qlinear_w8a8_attn", M=1024, N=1280, K=1280, rows_per_image=1024, tkv=77,
                  k_batch_stride=77 * 1280, k_row_stride=1280, v_batch_stride=77 * 1280, v_row_stride=1280,
                  softmax_scale=0.125, flags=0)
    halo = conv_entry(t, N=1, H=64, W=64, C=640, K=640)
    a512 = attention_entry(t, heads=1, head_dim=512, tq=1024, tkv=1024)
    a160 = attention_entry(t, heads=8, head_dim=160, tq=4096, tkv=4096)
    for entry, shape, name in ((rows, {}, "tile20"), (pp, {}, "persistent"), (att, {}, "gemm_attn"),
                               (halo, {}, "halo"), (a512, {}, "attn512"), (a160, {}, "attn160"),
                               (gn1, GN_TAB, "gn_silu"), (geglu, GEGLU_TAB, "geglu"), (gemm_geglu, {}, "gemm_geglu")):
        for i, dev in enumerate((0, 0, 1)):
            lib.launch_trace_set_device(dev)
            entry.case(f"seq_optin_{name}_{i}_device{dev}", **shape)
    lib.launch_trace_set_device(0)


def attention_entry(t, name="mixdq_attention_f16", heads=10, head_dim=64, tq=1024, tkv=1024, **more):
    w = heads * head_dim
    return t.entry(name, batch=2, heads=heads, head_dim=head_dim, tq=tq, tkv=tkv, q_batch_stride=tq * w,
                   q_row_stride=w, k_batch_stride=tkv * w, k_row_stride=w, v_batch_stride=tkv * w, v_row_stride=w,
                   out_batch_stride=tq * w, out_row_stride=w, softmax_scale=0.125, out_scale_inv_or_null=None,
                   out_zero_point_or_null=None, flags=0, **more)


def conv_entry(t, **shape):
    return t.entry("mixdq_qconv2d_w8a8_table", R=3, S=3, stride=1, pad=1, residual_f16_or_null=None,
                   residual_row_div=1, flags=0, **shape)


QUANT = (("f16", {}), ("q", dict(out_scale_inv_or_null=ptr(30), out_zero_point_or_null=ptr(31))),
         ("q_a4", dict(out_scale_inv_or_null=ptr(30), out_zero_point_or_null=ptr(31), flags=A4_0)))


def norm_cases(t):
    gn1, gn2, gn3, ln, geglu = norm_entries(t)
    # GroupNorm: HW = 64 (the apply blocks reduce the partials themselves), 4096 (finalize launch), 16384 (table)
    for hw, silu, (f, fl), outs in itertools.product((64, 4096, 16384), (0, 1), flag_cases([(FLAG_UNFUSED, "unfused")]),
                                                     ("both", "q", "f16")):
        o = {"q": dict(out_f16_or_null=None), "f16": dict(out_q_or_null=None)}.get(outs, {})
        gn3.case(f"hw{hw}_silu{silu}_{fl}_{outs}", HW=hw, apply_silu=silu, flags=f, **o)
    gn3.case("batch8", N=8)
    gn3.case("one_source", C1=640, x2_nhwc_f16_or_null=None, raw_q=t.host(ctypes.c_void_p, [ptr(44), 0]))
    for silu, (f, fl) in itertools.product((0, 1), flag_cases([(FLAG_UNFUSED, "unfused")])):     # below the table's threshold
        gn3.case(f"c320_hw4096_silu{silu}_{fl}", C=320, C1=160, apply_silu=silu, flags=f)
    gn3.case("no_raw", raw_q=None)
    gn3.case("c1280_g32", C=1280, C1=640, HW=1024)
    for hw in (64, 4096, 16384):
        gn1.case(f"hw{hw}", HW=hw)
        gn2.case(f"hw{hw}", HW=hw)
    gn1.case("c2048_hw256", C=2048, HW=256)
    # LayerNorm: every (rounding, n_out, FP16 copy, A4 slots) the entry point admits, at one and two rows per wave
    for m, (f, fl), n_out in itertools.product((5, 8192), flag_cases([(FLAG_UNFUSED, "unfused")]), (0, 1, 2, 3)):
        for h, a4m in itertools.product((0, 1) if n_out else (1,), range(1 << n_out)):
            ln.case(f"m{m}_{fl}_n{n_out}_h{h}_a4m{a4m}", M=m, n_out=n_out, flags=f | (a4m << 16),
                    **({} if h else dict(out_f16_or_null=None)))
    ln.case("c2048", C=2048)
    ln.case("c16", C=16)
    # GEGLU: arithmetic (small) and table (5 Mi outputs), each rounding and A4 form
    for (shape, sl), (f, fl) in itertools.product((({}, "small"), (GEGLU_TAB, "large")),
                                                  flag_cases([(FLAG_UNFUSED, "unfused"), (A4_0, "a4")])):
        geglu.case(f"{sl}_{fl}", flags=f, **shape)
        geglu.case(f"{sl}_{fl}_f16_only", flags=f, out_q_or_null=None, **shape)
    geglu.case("huge", M=1 << 20, D=5120)


def attention_cases(t):
    for d in (64, 40, 80, 160):
        heads = 10 if d == 64 else 8
        for tq, tkv, force, (ql, q) in itertools.product((256, 4096), (77, 128, 200, 4096), (0, 1, 2, 4), QUANT):
            e = attention_entry(t, heads=heads, head_dim=d, tq=tq, tkv=tkv)
            q = dict(q)
            q["flags"] = q.get("flags", 0) | forced(force)
            e.case(f"d{d}_tq{tq}_tkv{tkv}_force{force}_{ql}", **q)
    e = attention_entry(t, tq=77, tkv=77)
    e.case("causal", flags=FLAG_CAUSAL)
    e.case("causal_force1", flags=FLAG_CAUSAL | forced(1))
    e.case("causal_unfused", flags=FLAG_CAUSAL | FLAG_UNFUSED)
    attention_entry(t, heads=1, head_dim=512, tq=4096, tkv=4096).case("d512")
    attention_entry(t, heads=1, head_dim=512, tq=100, tkv=77).case("d512_ragged")
    pf = dict(prefetch_ptrs=t.host(ctypes.c_void_p, [ptr(60), ptr(61) + 8]),
              prefetch_bytes=t.host(ctypes.c_int64, [1 << 20, 4096]), n_prefetch=2)
    for tq, tkv, d in ((4096, 4096, 64), (256, 200, 64), (4096, 77, 64), (4096, 4096, 80)):
        heads = 10 if d == 64 else 8
        e = attention_entry(t, "mixdq_attention_f16_prefetch", heads=heads, head_dim=d, tq=tq, tkv=tkv, **pf)
        for ql, q in QUANT:
            e.case(f"d{d}_tq{tq}_tkv{tkv}_{ql}", **q)
        e.case(f"d{d}_tq{tq}_tkv{tkv}_no_payload", n_prefetch=0)


def quantize_cases(t):
    def dims(*v):
        return t.host(ctypes.c_int64, list(v))

    q = t.entry("mixdq_quantize_f16_i8", sizes=dims(1024), x_strides=dims(1), out_strides=dims(1), ndim=1, flags=0)
    routes = (("dense", dict()),
              ("dense_large", dict(sizes=dims(1 << 26))),
              ("dense_misaligned", dict(x_f16=ptr(1) + 2)),
              ("rows", dict(sizes=dims(4, 64), x_strides=dims(128, 1), out_strides=dims(64, 1), ndim=2)),
              ("scalar", dict(sizes=dims(4, 7), x_strides=dims(16, 1), out_strides=dims(7, 1), ndim=2)),
              ("transposed", dict(sizes=dims(64, 32), x_strides=dims(1, 64), out_strides=dims(32, 1), ndim=2)),
              ("empty", dict(sizes=dims(0))))
    for (name, over), (f, fl) in itertools.product(routes, flag_cases([(FLAG_UNFUSED, "unfused"), (A4_0, "a4")])):
        q.case(f"{name}_{fl}", flags=f, **over)
    e = t.entry("mixdq_embed_tokens_f16", B=2, T=77, C=768, V=49408)
    e.case("clip_l")
    e.case("large", B=64, T=77, C=1280)


def sampler_cases(t):
    base = dict(n_steps=4, guidance=7.5, n=65536, rows_per_image=1, row_stride=65536)
    masked = dict(channels=4)
    step = t.entry("mixdq_sampler_step", noise_stride=65536, **base)
    step_m = t.entry("mixdq_sampler_step_masked", noise_stride=65536, **base, **masked)
    rng = t.entry("mixdq_sampler_step_rng", n_image=16384, **base)
    rng_m = t.entry("mixdq_sampler_step_masked_rng", n_image=16384, **base, **masked)
    two = t.entry("mixdq_sampler_step_2m", **base)
    two_m = t.entry("mixdq_sampler_step_2m_masked", **base, **masked)
    for rows in (1, 2):
        r = dict(rows_per_image=rows)
        for e in (step, step_m):
            e.case(f"rows{rows}_noise", **r)
            e.case(f"rows{rows}_no_noise", noise_or_null=None, **r)
        for e in (rng, rng_m):
            e.case(f"rows{rows}_vec", **r)
            e.case(f"rows{rows}_odd_image", n_image=4, **r)
        two.case(f"rows{rows}", **r)
        two_m.case(f"rows{rows}", **r)
        for e in (step_m, rng_m, two_m):
            e.case(f"rows{rows}_channels8", channels=8, **r)
        step_m.case(f"rows{rows}_channels8_no_noise", channels=8, noise_or_null=None, **r)
        rng_m.case(f"rows{rows}_channels8_odd_image", channels=8, n_image=4, **r)
    for e in (step, step_m, rng, rng_m, two, two_m):
        e.case("n0", n=0)
        e.case("n_large", n=1 << 26, row_stride=1 << 26, **({"noise_stride": 1 << 26} if e in (step, step_m) else {}))
    off = dict(noise_or_null=None, seeds_or_null=None, hist_or_null=None, first_or_null=None, z=None, noise0=None,
               mask=None, blend=None)
    s3 = t.entry("mixdq_sampler_step3", table_width=4, n_steps=4, guidance=7.5, image_guidance=1.5, n=65536,
                 row_stride=65536, noise_stride=65536, n_image=16384, channels=4, **off)
    on_mask = dict(z=ptr(70), noise0=ptr(71), mask=ptr(72), blend=ptr(73))
    for ml, m in (("", {}), ("_masked", on_mask), ("_masked8", dict(on_mask, channels=8))):
        s3.case(f"plain{ml}", **m)
        s3.case(f"noise{ml}", noise_or_null=ptr(74), **m)
        s3.case(f"rng{ml}", seeds_or_null=ptr(75), **m)
        s3.case(f"rng_odd_image{ml}", seeds_or_null=ptr(75), n_image=4, **m)
        s3.case(f"2m{ml}", table_width=8, hist_or_null=ptr(76), first_or_null=ptr(77), **m)
    r = t.entry("mixdq_randn_f32", B=2, n_image=16384, stream=3, step=5)
    r.case("vec")
    r.case("odd", n_image=16383)
    r.case("large", B=64, n_image=1 << 22)
    t.entry("mixdq_rng_normals_from_bits", n_quads=4096).case("quads")


def image_cases(t):
    dtypes = ((0, "u8"), (1, "f16"), (2, "f32"))
    img = dict(sb=3 * 64 * 64, sc=64 * 64, sh=64, sw=1)
    msk = dict(mb=64 * 64, mh=64, mw=1)
    ing = t.entry("mixdq_image_to_nhwc8_f16", dtype=0, B=2, C=3, H=64, W=64, **img)
    ing_m = t.entry("mixdq_image_to_nhwc8_f16_masked", dtype=0, mask_dtype=0, B=2, C=3, H=64, W=64, **img, **msk)
    for d, dl in dtypes:
        ing.case(dl, dtype=d)
        for m, ml in dtypes:
            ing_m.case(f"{dl}_mask_{ml}", dtype=d, mask_dtype=m)
    ing.case("large", B=8, H=1024, W=1024, sb=3 << 20, sc=1 << 20, sh=1024)
    lat = t.entry("mixdq_vae_latent_sample", pixels=4096, L=4, scaling_factor=0.13025)
    for L, (nl, n) in itertools.product((4, 8), (("noise", {}), ("mode", dict(noise_or_null=None)))):
        lat.case(f"L{L}_{nl}", L=L, **n)
    m2l = t.entry("mixdq_mask_to_latent", dtype=0, sb=64 * 64, sh=64, sw=1, B=2, H=64, W=64, mode=1)
    for (d, dl), (mode, ml, over) in itertools.product(dtypes, ((0, "nearest", {}), (1, "any_wide", {}),
                                                                (1, "any_strided", dict(sw=2, sh=128, sb=128 * 64)))):
        m2l.case(f"{dl}_{ml}", dtype=d, mode=mode, **over)
    comp = t.entry("mixdq_composite_u8", db=3 * 64 * 64, dc=64 * 64, dh=64, dw=1, ob=3 * 64 * 64, oc=1, oh=64 * 3,
                   ow=3, mask_dtype=0, B=2, H=64, W=64, **msk)
    for d, dl in dtypes:
        comp.case(f"mask_{dl}", mask_dtype=d)
    cond = t.entry("mixdq_inpaint_cond_f16", pixels=4096, L=4)
    cond.case("L4")
    cond.case("L4_misaligned", zl=ptr(2) + 4)
    cond.case("L5", L=5)
    ip = t.entry("mixdq_ip2p_cond_f16", B=2, pixels_per_image=4096, L=4, rows=1, scale=1.0)
    for rows, (ll, over) in itertools.product((1, 3), (("L4", {}), ("L4_misaligned", dict(moments_f16=ptr(1) + 4)),
                                                       ("L8", dict(L=8)))):
        ip.case(f"rows{rows}_{ll}", rows=rows, **over)
    taps = dict(Tx=4, Ty=4, Bt=1)
    rs = t.entry("mixdq_resample", dtype=0, src_mode=0, dst_kind=0, B=2, C=3, Hs=64, Ws=64, Hd=100, Wd=52, **img, **taps)
    for (d, dl), mode, kind in itertools.product(dtypes, (0, 1), (0, 1, 2)):
        rs.case(f"{dl}_mode{mode}_dst{kind}", dtype=d, src_mode=mode, dst_kind=kind)
    rs.case("per_image_taps", Bt=2)
    paste = t.entry("mixdq_resample_paste_u8", db=3 * 64 * 64, dc=64 * 64, dh=64, dw=1, Hm=64, Wm=64, mask_dtype=0,
                    mask_mode=0, Ht=100, Wt=52, B=2, H=128, W=128, mb=128 * 128, mh=128, mw=1, **taps)
    for d, dl in dtypes:
        paste.case(f"binary_{dl}", mask_dtype=d)
    paste.case("soft_u8", mask_mode=1)
    bbox = t.entry("mixdq_mask_bbox", dtype=0, sb=64 * 64, sh=64, sw=1, B=2, H=64, W=64)
    dil = t.entry("mixdq_mask_dilate_u8", dtype=0, sb=64 * 64, sh=64, sw=1, B=2, H=64, W=64, radius=3)
    for d, dl in dtypes:
        bbox.case(dl, dtype=d)
        dil.case(dl, dtype=d)
    dil.case("large", B=64, H=1024, W=1024, sb=1 << 20, sh=1024)


def gemm_cases(t):
    lib = t.lib
    all_ids, f16_ids, grouped_ids, aq_ids, halo_ids = (tile_ids(lib, f) for f in (0, 1, 2, 3, 5))
    lin = dict(group_rows=0, group_stride=0, group_offset=0, residual_f16_or_null=None, residual_row_div=1, flags=0)
    # K tails (no whole K-tile of 64 or 128) take the one-phase staging; packed W2 (K % 64 == 0) gets there only
    # through operand offsets beyond 32 bits
    slow = {0: dict(K=1296), FLAG_W4: dict(K=1312), FLAG_W2: dict(M=1 << 26)}
    rows = t.entry("mixdq_qlinear_w8a8_rows", M=1024, N=1280, K=1280, **lin)
    for (w, wl), i in itertools.product(WBITS, all_ids):
        rows.case(f"{wl}_tile{i}", flags=w | forced(i))
        rows.case(f"{wl}_tile{i}_k_tail", flags=w | forced(i), **slow[w])
    for (w, wl), (M, N, K) in itertools.product(WBITS, ((64, 1280, 1280), (1024, 1280, 1280), (1024, 1280, 5120),
                                                        (4096, 640, 640), (4096, 640, 2560), (8192, 1280, 1280),
                                                        (8192, 10240, 1280), (32768, 640, 640), (16384, 320, 1280))):
        rows.case(f"{wl}_auto_{M}x{N}x{K}", M=M, N=N, K=K, flags=w)
    rows.case("unfused_no_bias", flags=FLAG_UNFUSED, bias_f16_or_null=None)
    rows.case("rowmap", group_rows=76, group_stride=77, group_offset=1, M=152)
    rows.case("residual", residual_f16_or_null=ptr(20))
    rows.case("persistent_rowmap", M=8192, N=10240, group_rows=76, group_stride=77, group_offset=1)
    rows.case("persistent_k128", M=8192, N=10240, K=128)
    rows.case("generic_k24", K=24)
    rows.case("generic_misaligned", A=ptr(1) + 4)
    rows.case("generic_large", K=24, M=1 << 20)
    t.entry("mixdq_qlinear_w8a8", M=1024, N=1280, K=1280, flags=0).case("plain")

    geglu = t.entry("mixdq_qlinear_w8a8_geglu", M=1024, N=2560, K=640, flags=0)
    for (w, wl), i in itertools.product(WBITS, all_ids):
        geglu.case(f"{wl}_tile{i}", flags=w | forced(i))
    for (w, wl), (M, N, K) in itertools.product(WBITS, ((1024, 10240, 1280), (4096, 5120, 640), (8192, 10240, 1280))):
        geglu.case(f"{wl}_auto_{M}x{N}x{K}", M=M, N=N, K=K, flags=w)
    geglu.case("k_tail", K=656)

    grouped = t.entry("mixdq_qlinear_w8a8_grouped", ngroups=70, M=154, max_N=1280, K=2048, group_rows=0,
                      group_stride=0, group_offset=0, flags=0)
    for (w, wl), i in itertools.product(WBITS, grouped_ids):
        grouped.case(f"{wl}_tile{i}", flags=w | forced(i))
        grouped.case(f"{wl}_tile{i}_k_tail", flags=w | forced(i), **{0: dict(K=2064), FLAG_W4: dict(K=2080),
                                                                      FLAG_W2: dict(M=1 << 26)}[w])

    for w, wl in WBITS:
        grouped.case(f"{wl}_auto_m64", M=64, flags=w)
        grouped.case(f"{wl}_auto_m154", flags=w)

    att = t.entry("mixdq_qlinear_w8a8_attn", M=1024, N=1280, K=1280, rows_per_image=1024, tkv=77,
                  k_batch_stride=77 * 1280, k_row_stride=1280, v_batch_stride=77 * 1280, v_row_stride=1280,
                  softmax_scale=0.125, flags=0)
    for (w, wl), (ql, q) in itertools.product(WBITS, QUANT):
        q = dict(q)
        q["flags"] = q.get("flags", 0) | w
        att.case(f"{wl}_{ql}", **q)
    att.case("a4_without_quantizer", flags=A4_0, out_scale_inv_or_null=None, out_zero_point_or_null=None)

    aq = t.entry("mixdq_qlinear_f16in_w8a8", lda=1280, M=1024, N=1280, K=1280, **lin)
    for (w, wl), i in itertools.product(WBITS[:2], aq_ids):
        aq.case(f"{wl}_tile{i}", flags=w | forced(i))
    for (w, wl), (M, N, K) in itertools.product(WBITS[:2], ((1024, 1280, 1280), (4096, 640, 640), (4096, 640, 320),
                                                            (64, 1280, 1280), (16384, 320, 320))):
        aq.case(f"{wl}_auto_{M}x{N}x{K}", M=M, N=N, K=K, lda=K, flags=w)
    aq.case("rowmap", flags=FLAG_A_ROWMAP, group_rows=76, group_stride=77, group_offset=1, M=152)
    aq.case("k_tail", K=1296, lda=1296)

    arrays = dict(scale_inv=t.host(ctypes.c_void_p, [ptr(50), ptr(51), ptr(52)]),
                  zero_point=t.host(ctypes.c_void_p, [ptr(53), ptr(54), ptr(55)]),
                  out_q=t.host(ctypes.c_void_p, [ptr(56), ptr(57), ptr(58)]))
    ln = t.entry("mixdq_qlinear_w8a8_ln", M=1024, N=1280, K=1280, residual_row_div=1, eps=1e-5, n_out=1, flags=0,
                 **arrays)
    for i, n_out in itertools.product(LN_TILE_IDS, (0, 1, 3)):
        ln.case(f"tile{i}_n{n_out}", flags=forced(i), n_out=n_out)
    ln.case("auto_1024x1280x1280")
    ln.case("auto_4096x640x640", M=4096, N=640, K=640)
    ln.case("auto_2048x1280x1280", M=2048)
    ln.case("grid_beyond_the_device", M=4096, flags=forced(56))
    t.entry("mixdq_qlinear_ln_status", status=t.host(ctypes.c_int, [0])).case("read")

    f16 = t.entry("mixdq_linear_f16", M=1024, N=1280, K=1280, residual_f16_or_null=None, residual_row_div=1, flags=0)
    acts = ((0, "plain"), (ACT_GELU, "gelu"), (ACT_QUICK_GELU, "quick_gelu"))
    for (a, al), i in itertools.product(acts, f16_ids):
        f16.case(f"{al}_tile{i}", flags=a | forced(i))
        f16.case(f"{al}_tile{i}_k_tail", flags=a | forced(i), K=648)
    for (a, al), (M, N, K) in itertools.product(acts, ((77, 768, 768), (154, 3072, 768), (1024, 1280, 1280),
                                                       (8192, 1280, 5120), (4096, 512, 512))):
        f16.case(f"{al}_auto_{M}x{N}x{K}", M=M, N=N, K=K, flags=a)
    for a, al in acts:
        f16.case(f"{al}_generic", K=4, flags=a)
    f16.case("residual", residual_f16_or_null=ptr(20))
    t.entry("mixdq_gemm_f16", M=64, N=64, K=64).case("debug_gemm")

    cf16 = t.entry("mixdq_conv2d_f16", N=1, H=64, W=64, C=128, K=128, R=3, S=3, stride=1, pad=1,
                   residual_f16_or_null=None, residual_row_div=1, flags=0)
    for i in f16_ids:
        cf16.case(f"tile{i}", flags=forced(i))
    cf16.case("auto")
    cf16.case("auto_512", H=512, W=512)
    cf16.case("generic_c4", C=4)
    cf16.case("upsample2x", flags=FLAG_UPS)
    cf16.case("pad_after_stride2", flags=PAD_AFTER, stride=2)
    cf16.case("1x1", R=1, S=1, pad=0)
    cf16.case("residual", residual_f16_or_null=ptr(20), residual_row_div=64 * 64)

    conv = conv_entry(t, N=1, H=60, W=60, C=320, K=320)          # (H, W not multiples of 8: outside the halo range)
    for (w, wl), i in itertools.product(WBITS[:2], all_ids):
        conv.case(f"{wl}_tile{i}", flags=w | forced(i))
    for w, wl in WBITS[:2]:
        conv.case(f"{wl}_auto", flags=w)
        conv.case(f"{wl}_1x1", flags=w, R=1, S=1, pad=0)
        conv.case(f"{wl}_stride2", flags=w, stride=2)
    conv.case("generic_c4", C=4)
    conv.case("generic_misaligned", X_nhwc=ptr(1) + 4)
    halo = conv_entry(t, N=1, H=64, W=64, C=640, K=640)
    for (w, wl), i in itertools.product(WBITS[:2], halo_ids):
        halo.case(f"{wl}_halo{i}", flags=w | forced(i))
        halo.case(f"{wl}_halo{i}_upsample2x", flags=w | forced(i) | FLAG_UPS)
    for (w, wl), (n, px, c, k) in itertools.product(WBITS[:2], ((1, 128, 320, 320), (1, 64, 640, 640), (1, 32, 1280, 1280),
                                                                (8, 32, 1280, 1280), (1, 128, 320, 4), (8, 128, 320, 4),
                                                                (1, 32, 1280, 640), (1, 64, 640, 320), (2, 16, 1280, 1280))):
        halo.case(f"{wl}_auto_n{n}_px{px}_c{c}_k{k}", N=n, H=px, W=px, C=c, K=k, flags=w)
    halo.case("residual_per_image", residual_f16_or_null=ptr(20), residual_row_div=64 * 64)
    full = t.entry("mixdq_qconv2d_w8a8", N=1, H=64, W=64, C=640, K=640, R=3, S=3, stride=1, pad=1, dilation=1, flags=0)
    full.case("padded")
    full.case("unpadded", pad=0)
    t.entry("mixdq_conv_border_table", K=640, R=3, S=3).case("3x3")
    t.entry("mixdq_conv_border_table", K=1 << 16, R=3, S=3).case("large")
    t.entry("mixdq_conv_zero_point_propagate", N=1, H=64, W=64, K=640, R=3, S=3, stride=1, pad=1).case("3x3")
    t.entry("mixdq_gelu_table").case("copy")
    t.entry("mixdq_silu_table", n_pos=t.host(ctypes.c_int, [0]), n_neg=t.host(ctypes.c_int, [0])).case("copy")


def record(which):
    """{"kernels": every registered kernel (sorted; the events index it), "cases": {case: "status|events"}} of this
    process under the knob set `which`.  The knob sets other than the default run the entry points they reach."""
    t = Tracer()
    sequences(t)
    norm_cases(t)
    attention_cases(t)
    if which == "default":
        quantize_cases(t)
        sampler_cases(t)
        image_cases(t)
        gemm_cases(t)
    else:
        t.entry("mixdq_qlinear_w8a8_rows", M=1024, N=1280, K=1280, group_rows=0, group_stride=0, group_offset=0,
                residual_f16_or_null=None, residual_row_div=1, flags=0).case("plain")
    bad = [c for c, v in t.out.items() if v.startswith(f"{ERR_LAUNCH}|")]
    assert not bad, f"cases {bad} answered MIXDQ_ERR_LAUNCH: the stand-in runtime refuses nothing"
    return {"kernels": t.kernels, "cases": t.out}


def run_children():
    """{"kernels": [...], "runs": {knob set: {case: "status|events"}}} from one fresh process per knob set."""
    build_trace_lib()
    out = {"knobs": KNOBS, "kernels": None, "runs": {}}
    for which, knobs in KNOBS.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("MIXDQ_") or k == "MIXDQ_TRACE_OBJ"}
        env.update(knobs)
        r = subprocess.run([sys.executable, "-m", "tests.launch_trace", which], cwd=ROOT, env=env, capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        got = json.loads(r.stdout)
        assert out["kernels"] in (None, got["kernels"])
        out["kernels"] = got["kernels"]
        out["runs"][which] = got["cases"]
    return out


def to_golden(trace):
    """The compact form that is committed: the runs under knobs keep only the cases that answer otherwise than the
    default run's case of the same name (or that it does not have)."""
    base = trace["runs"]["default"]
    runs = {w: (c if w == "default" else {k: v for k, v in c.items() if base.get(k) != v})
            for w, c in trace["runs"].items()}
    return dict(trace, runs=runs)


def from_golden(golden, case_names):
    """The full form of to_golden()'s: case_names = {knob set: the names of the cases it runs}."""
    base = golden["runs"]["default"]
    runs = {w: (c if w == "default" else {k: c.get(k, base.get(k)) for k in case_names[w]})
            for w, c in golden["runs"].items()}
    return dict(golden, runs=runs)


def launched(trace):
    """Indices (into trace["kernels"]) of the kernels that some recorded case launches."""
    seen = set()
    for cases in trace["runs"].values():
        for v in cases.values():
            seen.update(int(e[1:].split(":")[0]) for e in v.split("|", 1)[1].split(";") if e.startswith("L"))
    return seen


def unreached(trace):
    """The coverage remainder: registered kernels that no recorded case launches, by name."""
    hit = launched(trace)
    return [k for i, k in enumerate(trace["kernels"]) if i not in hit]


if __name__ == "__main__":
    json.dump(record(sys.argv[1]), sys.stdout)
