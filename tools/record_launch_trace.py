#!/usr/bin/env python3
"""Record tests/golden/launch_trace.json: what every launching entry point of the BUILT library launches, traced on
the CPU against a stand-in HIP runtime (tests/launch_trace.py has the cases; no GPU is touched).  Run on the objects
of the commit whose launch behaviour is to be pinned -- the one from BEFORE a refactor of the launch code, built in a
checkout of that commit:

    MIXDQ_TRACE_OBJ=<that checkout>/mixdq_amd/_obj python tools/record_launch_trace.py

Prints the coverage: kernels registered, kernels some case launches, and the remainder, which has to be what
tests/golden/launch_trace_unreached.json lists with a reason each.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import launch_trace as lt  # noqa: E402


def main():
    trace = lt.run_children()
    with open(lt.GOLDEN, "w") as f:
        json.dump(lt.to_golden(trace), f, separators=(",", ":"))
        f.write("\n")
    print(lt.GOLDEN, os.path.getsize(lt.GOLDEN), "bytes;", {w: len(c) for w, c in trace["runs"].items()}, "cases")
    rest = lt.unreached(trace)
    print(f"kernels: {len(trace['kernels'])} registered, {len(lt.launched(trace))} launched, {len(rest)} not reached")
    for k in rest:
        print("  not reached:", k)


if __name__ == "__main__":
    main()
