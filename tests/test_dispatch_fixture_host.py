"""The host side of the GEMM / conv dispatch answers what it answered when tests/golden/select_ids.json and
status_matrix.json were recorded (tools/record_dispatch_fixtures.py): every tile-selection query over the grid, and
the status of every call the Linear entry points settle before their first HIP call.  No GPU."""
import json
import os

import pytest

from tests import dispatch_fixture as df


@pytest.fixture(scope="module")
def answers():
    return df.run_child()


def _golden(name):
    with open(os.path.join(df.GOLDEN, name)) as f:
        return json.load(f)


def test_selection_queries_answer_as_recorded(answers):
    want, got = _golden("select_ids.json"), answers["select_ids.json"]
    assert (want["M"], want["N"], want["K"]) == (list(df.MS), list(df.NS), list(df.KS))
    assert sorted(got["answers"]) == sorted(want["answers"])
    for query, recorded in want["answers"].items():
        diff = [i for i, (a, b) in enumerate(zip(got["answers"][query], recorded)) if a != b]
        assert len(got["answers"][query]) == len(recorded) and not diff, (query, diff[:8])


def test_refused_calls_return_the_recorded_status(answers):
    want, got = _golden("status_matrix.json"), answers["status_matrix.json"]
    assert sorted(got) == sorted(want)
    for entry, cases in want.items():
        assert got[entry] == cases, (entry, {c: (got[entry].get(c), st) for c, st in cases.items()
                                             if got[entry].get(c) != st})
