#!/usr/bin/env python3
"""Record tests/golden/select_ids.json and status_matrix.json from the BUILT library (tests/dispatch_fixture.py
has the grid and the cases; no GPU is touched).  Run on the library of the commit whose host behaviour is to be
pinned -- the one from BEFORE a refactor of the dispatch code, built in a checkout of that commit:

    MIXDQ_HIP_LIB=<that checkout>/mixdq_amd/libmixdq_hip.so python tools/record_dispatch_fixtures.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dispatch_fixture as df  # noqa: E402


def main():
    for name, content in df.run_child().items():
        path = os.path.join(df.GOLDEN, name)
        with open(path, "w") as f:
            json.dump(content, f, separators=(",", ":"))
            f.write("\n")
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
