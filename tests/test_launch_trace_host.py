"""Every launching entry point launches what it launched when tests/golden/launch_trace.json was recorded
(tools/record_launch_trace.py): the same kernel instantiation, grid, block and dynamic LDS, the same LDS opt-ins per
device, the same table initialisations under a stream capture and outside one.  Traced on the CPU against a stand-in
HIP runtime (tests/launch_trace.py); no GPU."""
import json

import pytest

from tests import launch_trace as lt


@pytest.fixture(scope="module")
def trace():
    return lt.run_children()


@pytest.fixture(scope="module")
def golden(trace):
    with open(lt.GOLDEN) as f:
        return lt.from_golden(json.load(f), {w: list(c) for w, c in trace["runs"].items()})


def test_the_same_kernels_are_registered(trace, golden):
    got, want = set(trace["kernels"]), set(golden["kernels"])
    assert got == want, {"new": sorted(got - want)[:8], "gone": sorted(want - got)[:8]}


def test_every_call_launches_what_was_recorded(trace, golden):
    assert trace["knobs"] == golden["knobs"]

    def named(events, kernels):          # the kernel indices of an answer as names: comparable across kernel lists
        status, ev = events.split("|", 1)
        out = []
        for e in ev.split(";"):
            if e[:1] in ("L", "A"):
                i, _, rest = e[1:].partition(":")
                e = f"{e[0]} {kernels[int(i)]} {rest}"
            out.append(e)
        return status, out

    for which, want in golden["runs"].items():
        got = trace["runs"][which]
        assert sorted(got) == sorted(want), (which, sorted(set(got) ^ set(want))[:8])
        diff = {c: (named(got[c], trace["kernels"]), named(v, golden["kernels"])) for c, v in want.items()
                if named(got[c], trace["kernels"]) != named(v, golden["kernels"])}
        assert not diff, (which, len(diff), dict(list(diff.items())[:3]))


def test_no_case_fails_to_launch(trace):
    bad = [(w, c) for w, cases in trace["runs"].items() for c, v in cases.items() if v.startswith(f"{lt.ERR_LAUNCH}|")]
    assert not bad, bad[:8]


def test_every_registered_kernel_is_launched_or_listed(trace):
    with open(lt.UNREACHED) as f:
        listed = json.load(f)["unreached"]
    assert all(reason.strip() for reason in listed.values())
    assert sorted(lt.unreached(trace)) == sorted(listed)
