"""bench.py on the GPU, on the TINY harness network: `--steps` is the number of timed steps the line reports, and
`--dump-outputs DIR` writes what the timed path returned in its last step -- the same values on every run with the
same arguments, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_tiny(out_dir, steps):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--tiny", "--px", "512",
                           "--steps", str(steps), "--warmup", "1", "--no-fp16", "--no-cpu-baseline", "--no-roofline",
                           "--dump-outputs", str(out_dir)],
                          env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dump_outputs_is_the_timed_step_and_repeats(tmp_path):
    outs = []
    for run, steps in (("a", 3), ("b", 5)):
        line = _bench_tiny(tmp_path / run, steps)
        assert line["steps"] == steps and line["ms_per_step"] > 0
        assert line["dump_outputs"]["arrays"] == {"sample": {"shape": [1, 4, 64, 64], "elements": 4 * 64 * 64,
                                                             "sampled": False}}
        got = np.load(tmp_path / run / "sample.npy")
        assert got.dtype == np.float32 and got.shape == (1, 4, 64, 64)
        assert np.isfinite(got).all() and np.abs(got).max() > 0
        outs.append(got)
    # same inputs, same network, one timestep: the step count does not change what a step computes
    assert np.array_equal(outs[0], outs[1])
