"""What mixdq_sampler_step_rescaled LAUNCHES, recorded without a GPU as tests/launch_trace.py records the other entry
points: for rows 2 / 3 x order 1 / 2 x noise 0..3 x mask 0..2 (the combinations that exist) the instantiation of the
statistics and the step kernel and the exact grid (ceil(n_image / 2048), images); the refusals of the entry point; and
that the objects directly inside mixdq_amd/_obj/ register exactly the kernels they registered before this entry point
existed (its unit's object lives in _obj/ext/).

The stand-in runtime (tests/launch_trace_runtime.cpp) is linked against _obj/*.o plus _obj/ext/*.o into
_obj/ext/libmixdq_trace_rescale.so.  `python -m tests.test_launch_trace_rescale_host <environment>` is the child process
(the combine knob is read once per process); `... --record` rewrites tests/golden/launch_trace_rescale.json."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from tests import launch_trace as lt

EXT = os.path.join(lt.OBJ, "ext")
TRACE_LIB = os.path.join(EXT, "libmixdq_trace_rescale.so")
GOLDEN = os.path.join(lt.ROOT, "tests", "golden", "launch_trace_rescale.json")
ENVIRONMENTS = {"default": {}, "combine_launch": {"MIXDQ_RESCALE_COMBINE_LAUNCH": "1"}}
INVALID, ALIGNMENT = 1, 2
CHUNK = 2048


def build_trace_lib():
    objs = sorted(os.path.join(d, f) for d in (lt.OBJ, EXT) for f in os.listdir(d) if f.endswith(".o"))
    assert any(o.startswith(EXT) for o in objs), f"no objects under {EXT}: run mixdq_amd.build.build() first"
    deps = objs + [lt.RUNTIME_SRC]
    if not os.path.exists(TRACE_LIB) or any(os.path.getmtime(d) > os.path.getmtime(TRACE_LIB) for d in deps):
        tmp = TRACE_LIB + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-o", tmp,
                               lt.RUNTIME_SRC] + objs)
        os.replace(tmp, TRACE_LIB)
    return TRACE_LIB


class Tracer(lt.Tracer):
    """lt.Tracer over the library with the extension objects.  Both sampler units register a sampler_advance_kernel of
    their own under one name: the kernel list is a set."""

    def __init__(self):
        self.lib = ctypes.CDLL(build_trace_lib())
        self.lib.launch_trace_take.restype = ctypes.c_char_p
        self.lib.launch_trace_kernels.restype = ctypes.c_char_p
        self.sig = lt.signatures()
        self.kernels = sorted(set(self.lib.launch_trace_kernels().decode().split()))
        self.index = {k: i for i, k in enumerate(self.kernels)}
        self.out = {}
        self.keep = []


def modes():
    """[(label, overrides)] of every legal (order, noise, mask); the noise-3 ones come with an n_image % 8 != 0."""
    on_mask = dict(z=lt.ptr(70), noise0=lt.ptr(71), mask=lt.ptr(72), blend=lt.ptr(73))
    odd = dict(n=2 * 2076, n_image=2076, row_stride=4152, noise_stride=4152)       # (n % 8 == 0: channels 4 and 8)
    out = []
    for ml, m in (("", {}), ("_masked", on_mask), ("_masked8", dict(on_mask, channels=8))):
        out.append((f"plain{ml}", m))
        out.append((f"noise{ml}", dict(m, noise_or_null=lt.ptr(74))))
        out.append((f"rng{ml}", dict(m, seeds_or_null=lt.ptr(75))))
        out.append((f"rng_odd_image{ml}", dict(m, seeds_or_null=lt.ptr(75), **odd)))
        out.append((f"2m{ml}", dict(m, table_width=8, hist_or_null=lt.ptr(76), first_or_null=lt.ptr(77))))
    return out


def record():
    t = Tracer()
    off = dict(noise_or_null=None, seeds_or_null=None, hist_or_null=None, first_or_null=None, z=None, noise0=None,
               mask=None, blend=None)
    e = t.entry("mixdq_sampler_step_rescaled", table_width=4, n_steps=4, guidance=7.5, image_guidance=1.5, rescale=0.7,
                rows_per_image=2, n=2 * 65536, n_image=65536, row_stride=2 * 65536, noise_stride=2 * 65536, channels=4,
                **off)
    for rows in (2, 3):
        for label, over in modes():
            e.case(f"rows{rows}_{label}", rows_per_image=rows, **over)
        # the shapes of tests/test_rescale_gpu.py: (chunks, images) = (1, 3), (2, 3), (2, 3), (4, 3), (32, 1)
        for n_image, images in ((252, 3), (2072, 3), (4096, 3), (6400, 3), (65536, 1)):
            n = n_image * images
            stride = (n + 7) // 8 * 8
            e.case(f"rows{rows}_n_image{n_image}_x{images}", rows_per_image=rows, n=n, n_image=n_image, row_stride=stride,
                   noise_stride=stride)
        e.case(f"rows{rows}_n0", rows_per_image=rows, n=0)
        e.case(f"rows{rows}_images_65535", rows_per_image=rows, n=8 * 65535, n_image=8, row_stride=8 * 65535)
    # the refusals of the entry point itself, each with everything else in order
    e.case("refuse_rows1", rows_per_image=1)
    e.case("refuse_rows4", rows_per_image=4)
    e.case("refuse_phi_negative", rescale=-0.125)
    e.case("refuse_phi_above_one", rescale=1.5)
    e.case("refuse_phi_nan", rescale=float("nan"))
    e.case("refuse_n_image_zero", n_image=0)
    e.case("refuse_n_not_a_multiple", n_image=65528)
    e.case("refuse_no_workspace", workspace=None)
    e.case("refuse_workspace_misaligned", workspace=lt.ptr(17) + 8)
    e.case("refuse_images_65536", n=8 * 65536, n_image=8, row_stride=8 * 65536)
    e.case("refuse_width", table_width=5)
    e.case("refuse_2m_with_noise", table_width=8, hist_or_null=lt.ptr(76), first_or_null=lt.ptr(77),
           noise_or_null=lt.ptr(74))
    e.case("refuse_noise_and_seeds", noise_or_null=lt.ptr(74), seeds_or_null=lt.ptr(75))
    e.case("refuse_hist_without_2m", hist_or_null=lt.ptr(76), first_or_null=lt.ptr(77))
    e.case("refuse_x_null", x=None)
    e.case("refuse_row_stride_short", row_stride=65536)
    e.case("refuse_partial_mask", z=lt.ptr(70))
    size = t.lib.mixdq_sampler_rescale_workspace_floats
    size.argtypes, size.restype = [ctypes.c_int64, ctypes.c_int64], ctypes.c_size_t
    sizes = {f"{n}/{k}": size(n, k) for n, k in ((65536, 65536), (8 * 65536, 65536), (756, 252), (6216, 2072), (2049, 2049),
                                                 (0, 8), (-8, 8), (8, 0), (9, 8))}
    used = sorted({int(ev[1:].split(":")[0]) for v in t.out.values() for ev in v.split("|", 1)[1].split(";")
                   if ev.startswith("L")})
    renumber = {old: new for new, old in enumerate(used)}

    def compact(v):
        status, events = v.split("|", 1)
        out = []
        for ev in events.split(";"):
            if ev.startswith("L"):
                i, _, rest = ev[1:].partition(":")
                ev = f"L{renumber[int(i)]}:{rest}"
            out.append(ev)
        return status + "|" + ";".join(out)
    return {"kernels": [t.kernels[i] for i in used], "all_kernels": t.kernels,
            "cases": {k: compact(v) for k, v in t.out.items()}, "workspace_floats": sizes}


def run_children():
    build_trace_lib()
    out = {"kernels": {}, "runs": {}, "workspace_floats": None, "all_kernels": None}
    for which, knobs in ENVIRONMENTS.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("MIXDQ_") or k == "MIXDQ_TRACE_OBJ"}
        env.update(knobs)
        r = subprocess.run([sys.executable, "-m", "tests.test_launch_trace_rescale_host", which], cwd=lt.ROOT, env=env,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        got = json.loads(r.stdout)
        out["kernels"][which], out["runs"][which] = got["kernels"], got["cases"]
        out["workspace_floats"], out["all_kernels"] = got["workspace_floats"], got["all_kernels"]
    return out


@pytest.fixture(scope="module")
def trace():
    return run_children()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _named(v, kernels):
    status, events = v.split("|", 1)
    out = []
    for ev in events.split(";"):
        if ev.startswith("L"):
            i, _, rest = ev[1:].partition(":")
            ev = f"L {kernels[int(i)]} {rest}"
        out.append(ev)
    return status, out


def test_every_call_launches_what_was_recorded(trace, golden):
    assert sorted(trace["runs"]) == sorted(golden["runs"]) == sorted(ENVIRONMENTS)
    for which, want in golden["runs"].items():
        got = trace["runs"][which]
        assert sorted(got) == sorted(want)
        diff = {c: (_named(got[c], trace["kernels"][which]), _named(v, golden["kernels"][which]))
                for c, v in want.items()
                if _named(got[c], trace["kernels"][which]) != _named(v, golden["kernels"][which])}
        assert not diff, (which, len(diff), dict(list(diff.items())[:3]))
    assert trace["workspace_floats"] == golden["workspace_floats"]


def _demangled(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return r.stdout.split("\n")[:len(names)]


def test_the_grids_are_exact_and_the_instantiations_are_the_modes(trace):
    """Not against the recording but against the rule: statistics <ROWS, n_image % 8 == 0>, [the factor launch], step
    <ROWS, ORDER, NOISE, MASK>, all on (ceil(n_image / 2048), images) with 256 lanes, then the advance on one lane."""
    for which, cases in trace["runs"].items():
        names = _demangled(trace["kernels"][which])
        seen = set()
        for label, over in modes():
            for rows in (2, 3):
                status, events = cases[f"sampler_step_rescaled/rows{rows}_{label}"].split("|", 1)
                assert status == "0", (label, status)
                ev = [e[1:].split(":") for e in events.split(";")]
                n_image, images = over.get("n_image", 65536), 2
                grid = f"{(n_image + CHUNK - 1) // CHUNK},{images},1"
                order = 2 if over.get("table_width") == 8 else 1
                noise = (2 if n_image % 8 == 0 else 3) if "seeds_or_null" in over else 1 if "noise_or_null" in over else 0
                mask = 0 if "z" not in over else 2 if over.get("channels") == 8 else 1
                want = [(f"sampler_rescale_stats_kernel<{rows}, {'true' if n_image % 8 == 0 else 'false'}>", grid, "256")]
                if which == "combine_launch":
                    want.append(("sampler_rescale_factor_kernel(", "1,1,1", "64"))
                want += [(f"sampler_step_rescaled_kernel<{rows}, {order}, {noise}, {mask}>", grid, "256"),
                         ("sampler_advance_kernel(", "1,1,1", "1")]
                assert len(ev) == len(want), (label, ev)
                for (i, g, block, lds), (kernel, wg, wb) in zip(ev, want):
                    assert kernel in names[int(i)] and g == wg and block == wb and lds == "0", (label, names[int(i)], g)
                seen.add((rows, order, noise, mask))
        assert len(seen) == 2 * (4 * 3 + 3)                # every instantiation of the step kernel is reached


def test_refusals(trace):
    for which, cases in trace["runs"].items():
        want = {"refuse_workspace_misaligned": ALIGNMENT}
        refused = {c: v for c, v in cases.items() if "/refuse_" in c}
        assert len(refused) == 17
        for c, v in refused.items():
            assert v == f"{want.get(c.split('/')[1], INVALID)}|", (c, v)      # the status, and nothing launched
        for rows in (2, 3):
            assert cases[f"sampler_step_rescaled/rows{rows}_n0"].count("L") == 1      # the advance alone
            assert cases[f"sampler_step_rescaled/rows{rows}_images_65535"].startswith("0|")
    ws = trace["workspace_floats"]
    assert ws["65536/65536"] == 4 * 32 + 1 and ws["524288/65536"] == 8 * (4 * 32 + 1) and ws["756/252"] == 3 * 5
    assert ws["6216/2072"] == 3 * 9 and ws["2049/2049"] == 9 and ws["0/8"] == 0
    assert ws["-8/8"] == 0 and ws["8/0"] == 0 and ws["9/8"] == 0


def test_the_recorded_objects_register_what_they_registered(trace):
    """The kernels of _obj/*.o alone are tests/golden/launch_trace.json's: everything this library has beyond them
    comes from the extension unit."""
    with open(lt.GOLDEN) as f:
        before = set(json.load(f)["kernels"])
    now = set(trace["all_kernels"])
    assert before <= now, sorted(before - now)[:4]
    new = _demangled(sorted(now - before))
    assert len(new) == 4 + 1 + 30, len(new)
    assert all("sampler_rescale_" in k or "sampler_step_rescaled_kernel<" in k for k in new), new[:4]


if __name__ == "__main__":
    if sys.argv[1] == "--record":
        got = run_children()
        with open(GOLDEN, "w") as f:
            json.dump({"knobs": ENVIRONMENTS, "kernels": got["kernels"], "runs": got["runs"],
                       "workspace_floats": got["workspace_floats"]}, f, indent=0, sort_keys=True)
            f.write("\n")
    else:
        json.dump(record(), sys.stdout)
