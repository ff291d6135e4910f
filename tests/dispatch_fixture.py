"""What the library's host code answers without touching the GPU: the tile-selection queries over a grid of
shapes, and the status every Linear entry point returns for calls it refuses (or accepts as empty) BEFORE its first
HIP call.  tools/record_dispatch_fixtures.py writes both into tests/golden/ (select_ids.json, status_matrix.json);
tests/test_dispatch_fixture_host.py runs `python -m tests.dispatch_fixture` in a fresh child process and compares.

Plain ctypes on the built library (MIXDQ_HIP_LIB or the in-tree one), no torch.  The pointers of the status cases
are dummies that are never dereferenced: multiples of 4096 where a call wants alignment, small integers where it is
to refuse a misaligned one.  Only cases whose return precedes the first launch, LDS opt-in or table
initialisation belong here; none may answer MIXDQ_ERR_LAUNCH (record() checks).
What the calls that DO launch launch is pinned by tests/launch_trace.py, on the CPU against a stand-in HIP runtime.
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# read once per process by the selection rules: the child process runs without them
RULE_ENV = ("MIXDQ_IGEMM_TUNE", "MIXDQ_IGEMM_PERSIST", "MIXDQ_LN_MAXK", "MIXDQ_LN_LOCAL", "MIXDQ_HALO_CONV",
            "MIXDQ_HALO_W4")

MS = (1, 64, 256, 1024, 4096, 8192, 16384, 32768)
NS = (4, 6, 80, 320, 640, 1280, 1920, 3840, 5120, 10240)
KS = (16, 20, 32, 64, 96, 320, 640, 1280, 1296, 2048, 2560, 5120, 6144, 10240)
HALO_PX = (32, 64, 128)
HALO_CH = (320, 640, 1280)
HALO_BATCH = (1, 8)

FLAG_W4, FLAG_W2 = 2, 16
ACT_GELU, ACT_QUICK_GELU = 64, 128
A4_0, A4_1, A4_2 = 1 << 16, 1 << 17, 1 << 18
ERR_LAUNCH = 4

_vp, _i64, _i32, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float


def load():
    path = os.environ.get("MIXDQ_HIP_LIB") or os.path.join(ROOT, "mixdq_amd", "libmixdq_hip.so")
    lib = ctypes.CDLL(path)
    sig = {
        "mixdq_igemm_select_id": [_i64, _i32, _i32, _i32],
        "mixdq_igemm_select_id_w4": [_i64, _i32, _i32, _i32],
        "mixdq_igemm_select_id_w2": [_i64, _i32, _i32, _i32],
        "mixdq_igemm_select_id_geglu": [_i64, _i32, _i32, _i32],
        "mixdq_igemm_select_id_geglu_w2": [_i64, _i32, _i32],
        "mixdq_igemm_select": [_i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
        "mixdq_qlinear_f16in_select_id": [_i64, _i32, _i32, _i32],
        "mixdq_qlinear_ln_select_id": [_i64, _i32, _i32],
        "mixdq_conv_halo_select_flags": [_i32] * 10,
        "mixdq_qlinear_w8a8_rows": [_vp] * 6 + [_i64, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _vp],
        "mixdq_qlinear_w8a8_geglu": [_vp] * 6 + [_i64, _i32, _i32, _vp, _vp, _i32, _vp],
        "mixdq_qlinear_w8a8_grouped": [_vp, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
        "mixdq_qlinear_w8a8_attn": [_vp] * 7 + [_i64, _i32, _i32, _i32, _i32, _i64, _i32, _i64, _i32, _f32, _vp, _vp,
                                                _i32, _vp],
        "mixdq_qlinear_f16in_w8a8": [_vp, _i64] + [_vp] * 7 + [_i64, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _i32,
                                                               _vp],
        "mixdq_qlinear_w8a8_ln": [_vp] * 6 + [_i64, _i32, _i32, _vp, _i64, _vp, _vp, _f32, _i32] + [_vp] * 5
                                 + [_i32, _vp],
        "mixdq_linear_f16": [_vp] * 4 + [_i64, _i32, _i32, _vp, _i64, _i32, _vp],
    }
    for name, args in sig.items():
        f = getattr(lib, name)
        f.argtypes, f.restype = args, _i32
    return lib


# ---------------------------------------------------------------------------------------------- selection
def select_answers(lib):
    """{query: flat list of answers in grid order}; the grid is the cross product MS x NS x KS (K fastest), each
    point asked as a Linear (k_align = k_total = K) and, where the query takes both, as a 3x3 conv (k_total = 9 K)."""
    out = {k: [] for k in ("select_id", "select_id_conv", "select_id_w4", "select_id_w4_conv", "select_id_w2",
                           "select_id_w2_conv", "select_id_geglu", "select_id_geglu_w4", "select_id_geglu_w2",
                           "select", "select_conv", "f16in_select_id", "f16in_select_id_w4", "ln_select_id")}
    tile = [ctypes.c_int() for _ in range(4)]
    refs = [ctypes.byref(t) for t in tile]

    def select(M, N, ka, kt):
        for t in tile:
            t.value = -7          # (an answer that leaves them untouched shows as -7)
        st = lib.mixdq_igemm_select(M, N, ka, kt, *refs)
        return [st] + [t.value for t in tile]

    for M, N, K in itertools.product(MS, NS, KS):
        out["select_id"].append(lib.mixdq_igemm_select_id(M, N, K, K))
        out["select_id_conv"].append(lib.mixdq_igemm_select_id(M, N, K, 9 * K))
        out["select_id_w4"].append(lib.mixdq_igemm_select_id_w4(M, N, K, K))
        out["select_id_w4_conv"].append(lib.mixdq_igemm_select_id_w4(M, N, K, 9 * K))
        out["select_id_w2"].append(lib.mixdq_igemm_select_id_w2(M, N, K, K))
        out["select_id_w2_conv"].append(lib.mixdq_igemm_select_id_w2(M, N, K, 9 * K))
        out["select_id_geglu"].append(lib.mixdq_igemm_select_id_geglu(M, N, K, 0))
        out["select_id_geglu_w4"].append(lib.mixdq_igemm_select_id_geglu(M, N, K, 1))
        out["select_id_geglu_w2"].append(lib.mixdq_igemm_select_id_geglu_w2(M, N, K))
        out["select"].extend(select(M, N, K, K))
        out["select_conv"].extend(select(M, N, K, 9 * K))
        out["f16in_select_id"].append(lib.mixdq_qlinear_f16in_select_id(M, N, K, 0))
        out["f16in_select_id_w4"].append(lib.mixdq_qlinear_f16in_select_id(M, N, K, 1))
        out["ln_select_id"].append(lib.mixdq_qlinear_ln_select_id(M, N, K))
    # the 3x3 / stride 1 / pad 1 halo shapes: batch x px x C x K x flags (0, W4, W2)
    out["halo_select_flags"] = [
        lib.mixdq_conv_halo_select_flags(n, px, px, C, K, 3, 3, 1, 1, flags)
        for n, px, C, K, flags in itertools.product(HALO_BATCH, HALO_PX, HALO_CH, HALO_CH, (0, FLAG_W4, FLAG_W2))]
    return out


# ---------------------------------------------------------------------------------------------- statuses
def _ptr(i):
    return 4096 * i           # an aligned dummy, distinct per operand


class _Entry:
    """One entry point: its argument names in order, a base call that passes every check, and cases as overrides."""

    def __init__(self, lib, name, order, base):
        self.fn, self.name, self.order, self.base, self.out = getattr(lib, name), name, order, base, {}
        assert set(order) == set(base), set(order) ^ set(base)

    def case(self, label, **over):
        assert set(over) <= set(self.base), over
        assert label not in self.out, label
        a = dict(self.base, **over)
        self.out[label] = self.fn(*(a[k] for k in self.order))


def _cfg(i):
    return i << 8


def status_answers(lib):
    """{entry point: {case: status}}.  Every base call is one that WOULD launch; each case changes what makes the
    entry point return before that."""
    res = {}
    keep = []                 # host arrays the LN cases point into

    # ---- mixdq_qlinear_w8a8_rows
    e = _Entry(lib, "mixdq_qlinear_w8a8_rows",
               ["A", "W", "bias0", "scale", "bias", "D", "M", "N", "K", "grows", "gstride", "goff", "res", "res_div",
                "flags", "stream"],
               dict(A=_ptr(1), W=_ptr(2), bias0=_ptr(3), scale=_ptr(4), bias=_ptr(5), D=_ptr(6), M=64, N=64, K=128,
                    grows=0, gstride=0, goff=0, res=None, res_div=1, flags=0, stream=None))
    for f, n in ((ACT_GELU, "gelu"), (ACT_QUICK_GELU, "quick_gelu"), (ACT_GELU | ACT_QUICK_GELU, "both")):
        e.case(f"act_{n}", flags=f)
    e.case("act_before_null", flags=ACT_GELU, A=None)
    for k in ("M", "N", "K"):
        e.case(f"negative_{k}", **{k: -1})
    e.case("M0", M=0)
    e.case("N0", N=0)
    e.case("M0_null", M=0, A=None)
    for k in ("A", "W", "bias0", "scale", "D"):
        e.case(f"null_{k}", **{k: None})
    e.case("rowmap_residual", grows=76, gstride=77, goff=1, res=_ptr(7))
    e.case("rowmap_residual_w4w2", grows=76, gstride=77, goff=1, res=_ptr(7), flags=FLAG_W4 | FLAG_W2)
    e.case("w4w2", flags=FLAG_W4 | FLAG_W2)
    e.case("K18", K=18)
    e.case("N6", N=6)
    e.case("w2_K32", K=32, flags=FLAG_W2)
    e.case("w2_K18", K=18, flags=FLAG_W2)
    e.case("w4_K16", K=16, flags=FLAG_W4)
    for k in ("A", "W", "D", "scale", "bias0", "res"):
        e.case(f"w4_misaligned_{k}", flags=FLAG_W4, **{k: 8})
        e.case(f"w2_misaligned_{k}", flags=FLAG_W2, **{k: 8})
    e.case("w4_misaligned_bias", flags=FLAG_W4, bias=4)
    e.case("w2_misaligned_bias", flags=FLAG_W2, bias=4)
    for w, n in ((0, "w8"), (FLAG_W4, "w4"), (FLAG_W2, "w2")):
        for i in (2, 90, 99, 255):
            e.case(f"{n}_forced_{i}", flags=w | _cfg(i))
    for i in (27, 42, 43, 44, 45, 56):
        e.case(f"w2_forced_{i}", flags=FLAG_W2 | _cfg(i))
    res[e.name] = e.out

    # ---- mixdq_qlinear_w8a8_geglu (everything before ensure_gelu_table)
    e = _Entry(lib, "mixdq_qlinear_w8a8_geglu",
               ["A", "W", "bias0", "scale", "bias", "out", "M", "N", "K", "sinv", "zp", "flags", "stream"],
               dict(A=_ptr(1), W=_ptr(2), bias0=_ptr(3), scale=_ptr(4), bias=_ptr(5), out=_ptr(6), M=64, N=64, K=128,
                    sinv=_ptr(7), zp=_ptr(8), flags=0, stream=None))
    for f, n in ((ACT_GELU, "gelu"), (ACT_QUICK_GELU, "quick_gelu"), (ACT_GELU | ACT_QUICK_GELU, "both")):
        e.case(f"act_{n}", flags=f)
    for f, n in ((A4_0, "a4_0"), (A4_1, "a4_1"), (A4_2, "a4_2")):
        e.case(n, flags=f)
    e.case("a4_before_negative", flags=A4_0, M=-1)
    for k in ("M", "N", "K"):
        e.case(f"negative_{k}", **{k: -1})
    e.case("M0", M=0)
    e.case("N0", N=0)
    for k in ("A", "W", "bias0", "scale", "out", "sinv", "zp"):
        e.case(f"null_{k}", **{k: None})
    e.case("w4w2", flags=FLAG_W4 | FLAG_W2)
    e.case("w4w2_before_shape", flags=FLAG_W4 | FLAG_W2, N=16)
    e.case("N16", N=16)
    e.case("N48", N=48)
    e.case("K24", K=24)
    e.case("misaligned_out", out=4)
    for k in ("A", "W", "scale", "bias0"):
        e.case(f"misaligned_{k}", **{k: 8})
    e.case("misaligned_bias", bias=4)
    res[e.name] = e.out

    # ---- mixdq_qlinear_w8a8_grouped
    e = _Entry(lib, "mixdq_qlinear_w8a8_grouped",
               ["A", "groups", "ngroups", "M", "N", "K", "grows", "gstride", "goff", "flags", "stream"],
               dict(A=_ptr(1), groups=_ptr(2), ngroups=3, M=64, N=64, K=128, grows=0, gstride=0, goff=0, flags=0,
                    stream=None))
    for f, n in ((ACT_GELU, "gelu"), (ACT_QUICK_GELU, "quick_gelu"), (ACT_GELU | ACT_QUICK_GELU, "both")):
        e.case(f"act_{n}", flags=f)
    for k in ("M", "N", "K", "ngroups"):
        e.case(f"negative_{k}", **{k: -1})
    e.case("M0", M=0)
    e.case("N0", N=0)
    e.case("ngroups0", ngroups=0)
    e.case("null_A", A=None)
    e.case("null_groups", groups=None)
    e.case("ngroups_65536", ngroups=65536)
    e.case("w4w2", flags=FLAG_W4 | FLAG_W2)
    for w, n in ((0, "w8"), (FLAG_W4, "w4"), (FLAG_W2, "w2")):
        for K in {0: (24, 40), FLAG_W4: (16, 48), FLAG_W2: (32, 96)}[w]:     # not whole pieces of that width
            e.case(f"{n}_K{K}", K=K, flags=w)
        e.case(f"{n}_N6", N=6, flags=w)
        e.case(f"{n}_misaligned_A", A=8, flags=w)
        for i in (1, 13, 70, 99):                      # ids of the INT8 table that the grouped family lacks, and none
            e.case(f"{n}_forced_{i}", flags=w | _cfg(i))
    e.case("w2_forced_56", flags=FLAG_W2 | _cfg(56))
    res[e.name] = e.out

    # ---- mixdq_qlinear_w8a8_attn (everything before launch_att)
    e = _Entry(lib, "mixdq_qlinear_w8a8_attn",
               ["A", "W", "bias0", "scale", "k", "v", "out", "M", "N", "K", "rpi", "tkv", "kbs", "krs", "vbs", "vrs",
                "sm_scale", "sinv", "zp", "flags", "stream"],
               dict(A=_ptr(1), W=_ptr(2), bias0=_ptr(3), scale=_ptr(4), k=_ptr(5), v=_ptr(6), out=_ptr(7), M=128,
                    N=128, K=128, rpi=64, tkv=77, kbs=77 * 128, krs=128, vbs=77 * 128, vrs=128, sm_scale=0.125,
                    sinv=_ptr(8), zp=_ptr(9), flags=0, stream=None))
    for f, n in ((ACT_GELU, "gelu"), (ACT_QUICK_GELU, "quick_gelu"), (ACT_GELU | ACT_QUICK_GELU, "both")):
        e.case(f"act_{n}", flags=f)
    for k in ("M", "N", "K"):
        e.case(f"negative_{k}", **{k: -1})
    e.case("rpi0", rpi=0)
    e.case("tkv0", tkv=0)
    e.case("M0", M=0)
    e.case("N0", N=0)
    for k in ("A", "W", "bias0", "scale", "k", "v", "out"):
        e.case(f"null_{k}", **{k: None})
    e.case("sinv_without_zp", zp=None)
    e.case("zp_without_sinv", sinv=None)
    e.case("w4w2", flags=FLAG_W4 | FLAG_W2)
    e.case("N64", N=64)
    e.case("K64", K=64)
    e.case("rpi32", rpi=32)
    e.case("M_not_whole_images", M=192, rpi=128)
    e.case("tkv129", tkv=129)
    e.case("M_K_4GiB", M=1 << 20, K=4096)
    e.case("N_K_4GiB", N=1 << 20, K=4096)
    for k in ("krs", "vrs", "kbs", "vbs"):
        e.case(f"{k}_4", **{k: 132})
    for k in ("A", "W", "k", "v", "bias0", "scale"):
        e.case(f"misaligned_{k}", **{k: 8})
    e.case("misaligned_out_q", out=4)
    e.case("misaligned_out_f16", out=8, sinv=None, zp=None)
    e.case("a4_1", flags=A4_1)
    e.case("a4_2", flags=A4_2)
    e.case("a4_0_a4_1", flags=A4_0 | A4_1)
    e.case("a4_1_w4", flags=A4_1 | FLAG_W4)
    e.case("a4_1_after_alignment", flags=A4_1, A=8)
    res[e.name] = e.out

    # ---- mixdq_qlinear_f16in_w8a8
    e = _Entry(lib, "mixdq_qlinear_f16in_w8a8",
               ["A", "lda", "sinv", "zp", "W", "bias0", "scale", "bias", "D", "M", "N", "K", "grows", "gstride",
                "goff", "res", "res_div", "flags", "stream"],
               dict(A=_ptr(1), lda=128, sinv=_ptr(2), zp=_ptr(3), W=_ptr(4), bias0=_ptr(5), scale=_ptr(6),
                    bias=_ptr(7), D=_ptr(8), M=64, N=64, K=128, grows=0, gstride=0, goff=0, res=None, res_div=1,
                    flags=0, stream=None))
    for f, n in ((ACT_GELU, "gelu"), (ACT_QUICK_GELU, "quick_gelu"), (ACT_GELU | ACT_QUICK_GELU, "both")):
        e.case(f"act_{n}", flags=f)
    for f, n in ((A4_0, "a4_0"), (A4_1, "a4_1"), (A4_2, "a4_2")):
        e.case(n, flags=f)
    for k in ("M", "N", "K"):
        e.case(f"negative_{k}", **{k: -1})
    e.case("lda_below_K", lda=64)
    e.case("M0", M=0)
    e.case("N0", N=0)
    for k in ("A", "sinv", "zp", "W", "bias0", "scale", "D"):
        e.case(f"null_{k}", **{k: None})
    e.case("w2", flags=FLAG_W2)
    e.case("w4w2", flags=FLAG_W4 | FLAG_W2)
    e.case("N6", N=6)
    e.case("K24", K=24, lda=24)
    e.case("w4_K16", K=16, lda=16, flags=FLAG_W4)
    e.case("lda_132", lda=132)
    for k in ("A", "W", "D", "scale", "bias0", "res"):
        e.case(f"misaligned_{k}", **{k: 8})
    e.case("misaligned_bias", bias=4)
    e.case("rowmap_residual", grows=76, gstride=77, goff=1, res=_ptr(9))
    e.case("rowmap_residual_forced_99", grows=76, gstride=77, goff=1, res=_ptr(9), flags=_cfg(99))
    e.case("K48_no_tile", K=48, lda=48)
    for w, n in ((0, "w8"), (FLAG_W4, "w4")):
        for i in (1, 3, 20, 25, 70, 99):               # ids of the INT8 table that the family lacks, and none
            e.case(f"{n}_forced_{i}", flags=w | _cfg(i))
    res[e.name] = e.out

    # ---- mixdq_qlinear_w8a8_ln
    def ptrs(*vals):
        a = (ctypes.c_void_p * 3)(*vals)
        keep.append(a)
        return ctypes.cast(a, ctypes.c_void_p)

    full = (_ptr(20), _ptr(21), _ptr(22))
    e = _Entry(lib, "mixdq_qlinear_w8a8_ln",
               ["A", "W", "bias0", "scale", "bias", "D", "M", "N", "K", "res", "res_div", "gamma", "beta", "eps",
                "n_out", "sinv", "zp", "outq", "out_f16", "workspace", "flags", "stream"],
               dict(A=_ptr(1), W=_ptr(2), bias0=_ptr(3), scale=_ptr(4), bias=_ptr(5), D=_ptr(6), M=1024, N=1280,
                    K=1280, res=_ptr(7), res_div=1, gamma=_ptr(8), beta=_ptr(9), eps=1e-5, n_out=0, sinv=None,
                    zp=None, outq=None, out_f16=_ptr(10), workspace=_ptr(11), flags=0, stream=None))
    for f, n in ((ACT_GELU, "gelu"), (ACT_QUICK_GELU, "quick_gelu"), (ACT_GELU | ACT_QUICK_GELU, "both")):
        e.case(f"act_{n}", flags=f)
    for f, n in ((A4_0, "a4_0"), (A4_1, "a4_1"), (A4_2, "a4_2")):
        e.case(n, flags=f)
    for k in ("M", "N", "K", "n_out"):
        e.case(f"negative_{k}", **{k: -1})
    e.case("n_out4", n_out=4)
    e.case("M0", M=0)
    e.case("N0", N=0)
    for k in ("A", "W", "bias0", "scale", "D", "gamma", "beta", "workspace"):
        e.case(f"null_{k}", **{k: None})
    e.case("no_output_at_all", out_f16=None)
    e.case("w4", flags=FLAG_W4)
    e.case("w2", flags=FLAG_W2)
    e.case("w4w2", flags=FLAG_W4 | FLAG_W2)
    e.case("N1920_no_tile", N=1920)
    e.case("N64_no_tile", N=64)
    e.case("K192_no_tile", K=192)
    e.case("K2560_no_tile", K=2560)
    e.case("M_K_4GiB", M=1 << 22, K=1024)
    e.case("shape_before_alignment", N=64, A=8)
    for k in ("A", "W", "D", "scale", "bias0", "res", "gamma", "beta", "out_f16", "workspace"):
        e.case(f"misaligned_{k}", **{k: 8})
    e.case("misaligned_bias", bias=4)
    e.case("n_out2_null_arrays", n_out=2)
    e.case("n_out2_null_member", n_out=2, sinv=ptrs(*full), zp=ptrs(full[0], None, None), outq=ptrs(*full))
    e.case("n_out2_misaligned_outq", n_out=2, sinv=ptrs(*full), zp=ptrs(*full), outq=ptrs(full[0], 4, None))
    for i in (1, 13, 37, 99):                          # ids of the INT8 table that the family lacks, and none
        e.case(f"forced_{i}", flags=_cfg(i))
        e.case(f"forced_{i}_n_out3", flags=_cfg(i), n_out=3, sinv=ptrs(*full), zp=ptrs(*full), outq=ptrs(*full))
    res[e.name] = e.out

    # ---- mixdq_linear_f16
    e = _Entry(lib, "mixdq_linear_f16",
               ["A", "W", "bias", "D", "M", "N", "K", "res", "res_div", "flags", "stream"],
               dict(A=_ptr(1), W=_ptr(2), bias=_ptr(3), D=_ptr(4), M=64, N=64, K=64, res=None, res_div=1, flags=0,
                    stream=None))
    for k in ("M", "N", "K"):
        e.case(f"negative_{k}", **{k: -1})
    e.case("M0", M=0)
    e.case("N0", N=0)
    for k in ("A", "W", "D"):
        e.case(f"null_{k}", **{k: None})
    e.case("w2", flags=FLAG_W2)
    e.case("w4w2", flags=FLAG_W4 | FLAG_W2)
    e.case("act_both", flags=ACT_GELU | ACT_QUICK_GELU)
    e.case("act_gelu_residual", flags=ACT_GELU, res=_ptr(5))
    e.case("act_quick_gelu_residual", flags=ACT_QUICK_GELU, res=_ptr(5))
    e.case("K_2_30", K=1 << 30)
    for f, n in ((0, "plain"), (ACT_GELU, "gelu"), (ACT_QUICK_GELU, "quick_gelu")):
        for i in (1, 3, 37, 70, 99):                   # ids of the INT8 table that the family lacks, and none
            e.case(f"{n}_forced_{i}", flags=f | _cfg(i))
    res[e.name] = e.out
    return res


def record():
    """Both fixtures of the loaded library, as the dict {file name: content}."""
    lib = load()
    status = status_answers(lib)
    for entry, cases in status.items():
        bad = [c for c, st in cases.items() if st == ERR_LAUNCH]
        assert not bad, f"{entry}: cases {bad} reached a HIP call; they do not belong in this fixture"
    lib.mixdq_build_csrc_sha16.restype = ctypes.c_char_p
    # (library_csrc_sha16: mixdq_amd.build.csrc_sha16() of the tree the answering library was built from -- of both
    #  files; what a fixture was recorded from can be checked against that commit's sources)
    return {"select_ids.json": dict(library_csrc_sha16=lib.mixdq_build_csrc_sha16().decode(), M=list(MS), N=list(NS), K=list(KS), halo_px=list(HALO_PX),
                                    halo_channels=list(HALO_CH), halo_batch=list(HALO_BATCH),
                                    answers=select_answers(lib)),
            "status_matrix.json": status}


def run_child():
    """record() of a fresh process (the rules read their environment once per process) without RULE_ENV."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in RULE_ENV}
    r = subprocess.run([sys.executable, "-m", "tests.dispatch_fixture"], cwd=ROOT, env=env, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout)


if __name__ == "__main__":
    assert not [v for v in RULE_ENV if v in os.environ], "run without " + ", ".join(RULE_ENV)
    json.dump(record(), sys.stdout)
