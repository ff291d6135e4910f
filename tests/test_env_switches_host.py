"""tests/env_switches.py on the CPU: the table is the census of the environment reads of csrc/ and of the package, every
row that names a test names one that exists and mentions the switch, and the child-process helper fails as it says.
No GPU, no built library."""
import os
import re

import pytest

from tests import env_switches as es
from tests import tile_map as tm


def test_the_table_is_the_census_of_the_c_side_reads():
    got = es.census_c()
    want = {(r["name"], r["site"]) for r in es.C_ROWS}
    # MIXDQ_HALO_CONV is read twice in igemm.hip (the launch's static and the query's getenv): one row
    assert got == want, {"without a row": sorted(got - want), "rows without a read": sorted(want - got)}
    assert len(got) >= 21
    # the helpers of csrc/common.h are the ones the census knows: a further one would read switches unseen
    text = open(os.path.join(es.CSRC, "common.h")).read()
    assert "inline int env_int(const char* name, int fallback)" in text
    assert "inline long long env_int64(const char* name, long long fallback)" in text
    assert "inline bool env_flag(const char* name, bool on_by_default)" in text
    assert set(re.findall(r"^inline [\w ]+? (env_\w+)\(", text, flags=re.M)) == {"env_int", "env_int64", "env_flag"}
    assert ("MIXDQ_GN_SILU_TAB_MIN", "fused_norm.hip") in got


def test_the_table_is_the_census_of_the_python_side_reads():
    got = es.census_py()
    want = {(r["name"], r["site"]) for r in es.PY_ROWS}
    assert got == want, {"without a row": sorted(got - want), "rows without a read": sorted(want - got)}
    # no other spelling of an environment read of one of the project's names hides from the census
    for base, _, files in os.walk(os.path.join(es.ROOT, "mixdq_amd")):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(base, f)).read()
                other = re.findall(r"(?:getenv\(|environ\[)\s*[\"']MIXDQ_", text)
                assert not other, (f, other)
                # ... and every `environ.get(` of one, in either kind of quotes, is one the census counted
                assert len(re.findall(r"environ\.get\(\s*[\"']MIXDQ_", text)) == len(es.PY_READ.findall(text)), f
    assert es.PY_READ.findall("os.environ.get('MIXDQ_X', '0')") == ["MIXDQ_X"]


def test_rows_are_complete_and_unique():
    names = [r["name"] for r in es.ROWS]
    assert len(set(names)) == len(names)
    for r in es.ROWS:
        assert r["read"] and r["alternative"] and r["relation"] and r["run"][0] in ("new", "existing", "not run"), r
        if r["run"][0] == "not run":
            assert len(r["run"][1]) > 20, r["name"]                      # a reason
        elif r["run"][0] == "new":
            assert r["values"], r["name"]
    # what cannot be told from outside a launch is said so: the tile order, the XCD map, the payload's policy
    hidden = {r["name"] for r in es.ROWS if not r["observable"]}
    assert {"MIXDQ_IGEMM_GM", "MIXDQ_ATTN_XCD", "MIXDQ_PREFETCH_NT", "MIXDQ_PREFETCH_DELAY"} <= hidden
    assert "MIXDQ_RESCALE_COMBINE_LAUNCH" not in hidden


@pytest.mark.parametrize("r", [r for r in es.ROWS if r["run"][0] != "not run"], ids=lambda r: r["name"])
def test_the_named_test_exists_and_mentions_the_switch(r):
    _, path, function = r["run"]
    text = es.function_text(path, function)
    assert text is not None, f"{path} has no function {function}"
    assert r["token"] in text, f"{path}::{function} does not mention {r['token']}"
    if r["run"][0] == "new":
        assert re.search(r"^def " + function + r"\(", open(os.path.join(es.ROOT, path)).read(), flags=re.M)
    if r["run"][0] == "new" and r["read"] not in (es.PY, es.PY_IMPORT):
        # a C-side row: the driver passes every value of the row to a child, as a quoted string beside the name (a
        # module constant's test sets the attribute, not the variable: its values are the switch's, not the test's)
        assert f'"{r["name"]}"' in text, r["name"]
        for v in r["values"]:
            if len(v) > 8:                          # (a long value may be a constant of the file)
                assert f'"{v}"' in open(os.path.join(es.ROOT, path)).read(), (r["name"], v)
            else:
                assert f'"{v}"' in text, (r["name"], v)


def test_children_select_only_cases_never_drivers():
    """A child runs `test_case_...` functions and tests of other files: no selection of this file's own tests can match
    a driver (which would start children of its own)."""
    text = open(os.path.join(es.ROOT, es.GPU)).read()
    drivers = [name for name, args in re.findall(r"^def (test_(?!case_)\w+)\(([^)]*)\)", text, flags=re.M)
               if "C" not in [a.strip() for a in args.split(",")]]          # (what takes the library runs in process)
    assert len(drivers) >= 9 and "test_tile_map_super_row_sizes" in drivers
    # a driver walks its values itself and stops at the first failing child: none is parametrized
    for d in drivers:
        assert "parametrize" not in es.function_text(es.GPU, d), d
    assert "timeout=120" in open(es.__file__).read()
    selections = re.findall(r"\"([^\"]*environment_is_what[^\"]*)\"", text)
    words = {w for w in re.findall(r"[A-Za-z_0-9\-]+", " ".join(selections)) if len(w) >= 6}
    assert "environment_is_what" in words and len(words) >= 10
    for d in drivers:
        assert not any(w in d for w in words), (d, sorted(w for w in words if w in d))
    assert "assert es.EXPECT not in os.environ" in text


def test_gm_children_run_every_configuration_once_per_form():
    from tests import tile_edges as te
    parts, seen = es.gm_edge_nodes()
    nodes = parts["linear"] + parts["geglu"] + parts["other"]
    assert len(nodes) == len(set(nodes)) and all(parts.values()) and len(nodes) == 93
    assert set(seen["linear"]) == set(seen["conv"]) == set(te.IGEMM)
    assert set(seen["geglu"]) == {c for c in te.IGEMM if te.geglu_admissible(c)}
    assert set(seen["f16in"]) == set(te.AQ) and set(seen["f16"]) == set(te.F16) and set(seen["grouped"]) == set(te.GROUPED)
    # three m-tiles wherever the form has such a case: super-rows 1 + 1 + 1 and 2 + 1 under gm = 1 and 2
    for form in ("linear", "geglu", "f16in", "f16", "pp_f16", "pp_residual"):
        assert set(seen[form].values()) == {3}, (form, seen[form])
        assert all(tm.paths(3, 1, gm)["second_super_row"] for gm in (1, 2)) and tm.paths(3, 1, 2)["partial_super_row"]
    # what tests/tile_edges.py gives the other forms: conv images of one or two m-tiles (one: nothing of the map under any
    # gm; two: a second super-row under gm = 1 only), two for every grouped configuration and for the persistent GEGLU case
    assert set(seen["conv"].values()) == {1, 2} and set(seen["grouped"].values()) == {2}
    assert set(seen["pp_geglu"].values()) == {2}
    assert tm.paths(2, 1, 1)["second_super_row"] and not tm.paths(2, 1, 2)["second_super_row"]
    assert not any(tm.paths(2, 1, 2).values()) and not any(tm.paths(1, 1, 1).values())
    # ... which is why the conv, grouped and GEGLU families of tests/tile_map.py run under the switch on 11 m-tiles
    assert {"conv", "grouped", "geglu", "pp71"} <= set(tm.FAMILIES)
    text = {p: open(os.path.join(es.ROOT, p)).read() for p in {n.split("::")[0] for n in nodes}}
    for n in nodes:
        path, rest = n.split("::")
        assert re.search(r"^def " + rest.split("[")[0] + r"\(", text[path], flags=re.M), n


def test_gm_rule_is_the_row_s_range():
    row = next(r for r in es.ROWS if r["name"] == "MIXDQ_IGEMM_GM")
    assert all(tm.gm_rule(int(v)) == int(v) for v in row["values"])
    assert tm.gm_rule(0) == 8 and tm.gm_rule(65) == 8


def test_expected_environment_round_trip(monkeypatch):
    env = {"MIXDQ_PREFETCH_BLOCKS": "8", "MIXDQ_IGEMM_TUNE": "300x256x256=35,300x320x256=42"}
    monkeypatch.setenv(es.EXPECT, es.expect_value(env))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert es.check_expected_env() == env
    monkeypatch.setenv("MIXDQ_PREFETCH_BLOCKS", "4")
    with pytest.raises(AssertionError):
        es.check_expected_env()
    monkeypatch.delenv(es.EXPECT)
    assert es.check_expected_env() == {}


def test_run_child_fails_on_status_signal_and_timeout(tmp_path, monkeypatch):
    """run_child on stand-in test files (no GPU): a passing child returns; a failing one and one killed by a signal
    fail the caller (the timeout is subprocess.run's own)."""
    d = tmp_path / "tests"
    d.mkdir()
    (d / "__init__.py").write_text("")
    body = "import os, signal, time, pytest\npytestmark = pytest.mark.gpu\n"
    (d / "test_ok.py").write_text(body + "def test_a():\n    assert os.environ['MIXDQ_X'] == '1'\n")
    (d / "test_bad.py").write_text(body + "def test_a():\n    assert False\n")
    (d / "test_sig.py").write_text(body + "def test_a():\n    os.kill(os.getpid(), signal.SIGKILL)\n")
    monkeypatch.setattr(es, "ROOT", str(tmp_path))
    out, dt = es.run_child({"MIXDQ_X": "1"}, ["tests/test_ok.py"], timeout=120)
    assert "1 passed" in out and dt > 0
    for target in ("tests/test_bad.py", "tests/test_sig.py"):
        with pytest.raises(AssertionError):
            es.run_child({"MIXDQ_X": "1"}, [target], timeout=120)
    assert "timeout=timeout" in open(es.__file__).read() and "TimeoutExpired" in open(es.__file__).read()
