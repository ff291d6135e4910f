"""bench.py's own N > 1 plumbing, on the CPU: `python bench.py --gpus 2` with no launcher must
start two ranks itself (fresh child processes, before any GPU call in the parent), shard the batch,
broadcast rank 0's quantized buffers and report n_gpus == 2 -- never a silent 1-GPU line.
`--host-only --tiny` is the harness check of that plumbing: no forward, no timing, value = null
(the product has no CPU path to time)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*flags, env_extra=None, timeout=600):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["MIXDQ_DIST_BACKEND"] = "gloo"
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--tiny", "--host-only",
                           *flags], env=env, capture_output=True, text=True, timeout=timeout)


def _line(proc):
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout
    return json.loads(lines[0])


def test_gpus_2_spawns_two_ranks_and_broadcasts():
    out = _line(_bench("--gpus", "2"))
    assert out["n_gpus"] == 2
    assert out["weight_broadcast_bytes"] > 0
    assert out["scaling"] == "weak" and out["config"]["per_gpu_batch"] == 1
    assert out["config"]["global_batch"] == 2
    assert out["value"] is None and out["host_only"] is True


def test_named_config_3_is_strong_scaling_over_the_ranks():
    out = _line(_bench("--gpus", "2", "--baseline-config", "3"))
    assert out["n_gpus"] == 2 and out["scaling"] == "strong"
    assert out["config"]["per_gpu_batch"] == 32 and out["config"]["global_batch"] == 64
    assert out["config"]["unet_forwards_per_image"] == 4


def test_world_size_mismatch_fails_loudly():
    proc = _bench("--gpus", "2", env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert proc.returncode != 0
    assert "--gpus 2 but WORLD_SIZE=1" in proc.stderr + proc.stdout


def test_a_failing_rank_fails_the_parent():
    # rank 1 cannot rendezvous with itself only: give the children a world of 2 but kill rank 1's
    # import by an impossible backend -> the parent must exit non-zero and print no JSON line
    proc = _bench("--gpus", "2", env_extra={"MIXDQ_DIST_BACKEND": "no-such-backend"}, timeout=300)
    assert proc.returncode != 0
    assert not [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mixdq_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_steps_below_one_is_refused():
    proc = _bench("--steps", "0")
    assert proc.returncode != 0 and "--steps must be at least 1" in proc.stderr


def test_dump_outputs_writes_float32_whole_when_it_fits(tmp_path):
    import numpy as np
    import torch
    b = _bench_module()
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(1)).half()
    info = b.dump_outputs(str(tmp_path), {"sample": x})
    got = np.load(tmp_path / "sample.npy")
    assert got.dtype == np.float32 and got.shape == (2, 4, 16, 16)
    assert np.array_equal(got, x.float().numpy())
    assert info == {"sample": {"shape": [2, 4, 16, 16], "elements": x.numel(), "sampled": False}}
    assert not (tmp_path / "sample_index.npy").exists()


def test_dump_outputs_samples_the_same_elements_within_the_budget(tmp_path):
    import numpy as np
    import torch
    b = _bench_module()
    x = torch.randn(64, 1000, generator=torch.Generator().manual_seed(2))
    budget = 12 * 1000                                   # room for 1000 (value, index) pairs, not 64000 values
    runs = []
    for d in ("a", "b"):
        info = b.dump_outputs(str(tmp_path / d), {"sample": x}, budget=budget)
        vals, idx = np.load(tmp_path / d / "sample.npy"), np.load(tmp_path / d / "sample_index.npy")
        assert info["sample"]["sampled"] and info["sample"]["shape"] == [64, 1000]
        assert vals.dtype == np.float32 and idx.dtype == np.float64
        assert vals.nbytes + idx.nbytes <= budget and vals.size == idx.size == info["sample"]["elements"]
        assert (np.diff(idx) > 0).all()
        assert np.array_equal(vals, x.numpy().reshape(-1)[idx.astype(np.int64)])
        runs.append(idx)
    assert np.array_equal(runs[0], runs[1])


def test_plain_run_drops_every_extra_leg_and_full_keeps_them(monkeypatch):
    b = _bench_module()
    legs = ("no_fp16", "no_roofline", "no_batch8", "no_dropin", "no_lnchain", "no_cpu_baseline")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1"])
    plain = b.parse_args()
    assert not plain.full and all(getattr(plain, k) for k in legs)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--full", "--no-batch8"])
    full = b.parse_args()
    assert full.full and full.no_batch8 and not any(getattr(full, k) for k in legs if k != "no_batch8")


def test_synthetic_unet_is_build_unet_bit_for_bit():
    import torch
    from mixdq_amd.unet import build_unet
    b = _bench_module()
    want, got = build_unet("cpu", cfg=b.TINY_CFG), b.build_synthetic_unet("cpu", cfg=b.TINY_CFG)
    assert not got.training
    sw, sg = want.state_dict(), got.state_dict()
    assert list(sw) == list(sg)
    for k in sw:
        assert sg[k].dtype == sw[k].dtype == torch.float16 and sg[k].stride() == sw[k].stride(), k
        assert torch.equal(sg[k].view(torch.int16), sw[k].view(torch.int16)), k


def test_conv2d_f64_sum_is_the_float64_convolution_rounded_through_fp32():
    # the indexing of the im2col GEMM (kernel taps, stride, padding, batch) against torch's own float64 convolution;
    # tests/test_bench_gpu.py compares it with F.conv2d on the GPU
    import torch
    import torch.nn.functional as F
    b = _bench_module()
    g = torch.Generator().manual_seed(3)
    for cin, cout, k, stride, pad, hw, n in ((4, 32, 3, 1, 1, 16, 1), (64, 48, 3, 2, 1, 17, 2),
                                             (96, 40, 1, 1, 0, 9, 1), (40, 24, 3, 1, 1, 8, 2)):
        cl = torch.channels_last
        x = (torch.randn(n, cin, hw, hw, generator=g) * 3).half().contiguous(memory_format=cl)
        w = (torch.randn(cout, cin, k, k, generator=g) * 0.05).half().contiguous(memory_format=cl)
        bias = (torch.randn(cout, generator=g) * 0.1).half()
        got = b.conv2d_f64_sum(x, w, bias, (stride, stride), (pad, pad), (1, 1))
        want = F.conv2d(x.double(), w.double(), None, stride, pad).float().half() + bias.view(1, -1, 1, 1)
        assert got.is_contiguous(memory_format=cl) and got.shape == want.shape
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
