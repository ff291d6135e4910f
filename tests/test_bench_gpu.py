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


def _deterministic(fn):
    import torch
    was = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        return fn()
    finally:
        torch.use_deterministic_algorithms(was[0], warn_only=was[1])


# the SDXL UNet's kinds of convolution at reduced sizes: conv_in, a resnet 3x3 with its 11520-long sums, a stride-2
# downsampler on an odd size, a 2560-channel 1x1 shortcut; activations with outliers, so that partial sums pass 32
@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,k,stride,hw,n", [(4, 320, 3, 1, 24, 1), (1280, 64, 3, 1, 8, 2),
                                                   (320, 96, 3, 2, 17, 1), (2560, 128, 1, 1, 8, 1)])
def test_conv2d_f64_sum_is_the_deterministic_conv(cin, cout, k, stride, hw, n):
    import torch
    import torch.nn.functional as F
    from tests.test_bench_cpu import _bench_module
    b = _bench_module()
    g = torch.Generator().manual_seed(cin + cout)
    cl = torch.channels_last
    x = torch.randn(n, cin, hw, hw, generator=g) * 2
    x.view(-1)[torch.randint(0, x.numel(), (x.numel() // 200,), generator=g)] *= 40
    x = x.half().cuda().contiguous(memory_format=cl)
    w = (torch.randn(cout, cin, k, k, generator=g) * 0.02).half().cuda().contiguous(memory_format=cl)
    bias = (torch.randn(cout, generator=g) * 0.02).half().cuda()
    pad = k // 2
    want = _deterministic(lambda: F.conv2d(x, w, bias, stride, pad))
    got = b.conv2d_f64_sum(x, w, bias, (stride, stride), (pad, pad), (1, 1))
    assert got.shape == want.shape and got.stride() == want.stride()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.gpu
def test_calibration_with_f64_sum_convs_is_the_stock_calibration():
    import torch
    from mixdq_amd.calib import calibrate
    from mixdq_amd.quantize_sdxl import example_inputs
    from tests.test_bench_cpu import _bench_module
    b = _bench_module()
    unet = b.build_synthetic_unet(torch.device("cuda", 0), cfg=b.TINY_CFG)
    inputs = example_inputs(1, 16, "cuda", seed=42)
    want = _deterministic(lambda: calibrate(unet, [inputs]))
    with b.Float64SumConvs(unet):
        got = _deterministic(lambda: calibrate(unet, [inputs]))
    assert all("forward" not in vars(m) for m in unet.modules())
    assert list(got) == list(want)
    for name in want:
        for k in want[name]:
            assert torch.equal(got[name][k].view(torch.int16), want[name][k].view(torch.int16)), (name, k)
