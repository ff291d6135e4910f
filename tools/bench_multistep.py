"""What the multistep solver costs per step: mixdq_sampler_step_2m against mixdq_sampler_step, and whole 'dpmpp_2m' runs
against 'euler' runs of the same length.

    python tools/bench_multistep.py [--repeats 7] [--out profiles/multistep_bench.txt]

One box, one process, medians of alternating runs.
  launch  the step launch pair (the step kernel + the one-thread advance behind it) at SDXL's latent size (4 x 128 x
          128 per image), batch 1 unguided and batch 8 guided: `--launches` back-to-back launches walking a 1000-step
          table from step 1 (second-order steps for the multistep kernel), timed with device events.
  run     Sampler.sample() on the SDXL UNet at 1024 px, uniform W8A8 + BOS, synthetic weights, the fused graph: 20
          guided steps at batch 8 and 4 steps at batch 1, 'dpmpp_2m' against 'euler' on the same inputs, host clock
          from the call to a device synchronise behind it.
The expectation: one more FP32 read and write of the state per step, lost behind a UNet forward.  Each `run` line says
whether the dpmpp_2m median exceeds the euler median by more than the euler runs' own spread (max - min).
This tool measures time only; what a step count costs in image quality needs real weights."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_sd15 import _commit, _lib_sha16  # noqa: E402


class _Cfg:
    def __init__(self, w, a):
        self.w_config, self.a_config = w, a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--tiny", action="store_true", help="the tiny UNet at latent 32 instead (a rehearsal, not a figure)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_multistep.py needs a GPU"
    import bench
    from mixdq_amd import Sampler, _C, cfgs
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.sampler import schedule
    from mixdq_amd.unet import build_unet, quantizable_layers
    dev = torch.device("cuda:0")
    head = {"tool": "bench_multistep", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
            "hip": torch.version.hip, "lib_csrc_sha16": _lib_sha16(_C), "commit": _commit(), "repeats": a.repeats,
            "launches": a.launches}
    lines = [json.dumps(head)]
    print(lines[0], flush=True)
    L = 32 if a.tiny else 128

    # ---- the launch pair ----------------------------------------------------------------------------------------
    def launch_case(B, rows, g):
        n = B * 4 * L * L
        s1, s2 = schedule("euler", 1000, "trailing"), schedule("dpmpp_2m", 1000, "trailing")
        assert (s2.coef[1:a.launches + 1, 5] != 0).all()
        x = torch.randn(n, device=dev)
        hist = torch.randn(n, device=dev)
        eps = torch.randn(rows * n, device=dev).half()
        inp = torch.zeros(rows * n, dtype=torch.float16, device=dev)
        tt = torch.from_numpy(s1.t_table).to(dev)
        c1, c2 = torch.from_numpy(s1.coef).to(dev), torch.from_numpy(s2.coef).to(dev)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        first = torch.zeros(1, dtype=torch.int32, device=dev)
        t_d = torch.zeros((), device=dev)
        fns = {"step": lambda: _C.sampler_step(x, eps, inp, c1, tt, step, t_d, g, rows),
               "step_2m": lambda: _C.sampler_step_2m(x, eps, inp, hist, c2, tt, step, first, t_d, g, rows)}
        us = {k: [] for k in fns}
        for rep in range(a.repeats + 2):                    # the first two trips are untimed
            for k, fn in fns.items():
                x.normal_()
                step.fill_(1)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    fn()
                e1.record()
                torch.cuda.synchronize(dev)
                assert int(step.item()) == 1 + a.launches
                if rep >= 2:
                    us[k].append(round(1e3 * e0.elapsed_time(e1) / a.launches, 3))
        med = {k: statistics.median(v) for k, v in us.items()}
        rec = {"case": f"launch_bs{B}_rows{rows}", "n": n, "us_per_launch_pair": us, "median_us": med,
               "spread_us": {k: round(max(v) - min(v), 3) for k, v in us.items()},
               "step_2m_minus_step_us": round(med["step_2m"] - med["step"], 3),
               "extra_bytes_per_step": 8 * n}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    launch_case(1, 1, 0.0)
    launch_case(8, 2, 7.5)

    # ---- whole runs ---------------------------------------------------------------------------------------------
    cfg = dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64) if a.tiny else None
    unet = build_unet(dev, cfg=cfg)
    inputs2 = example_inputs(2, L, dev, seed=42, cfg=cfg)
    ckpt = calibrate(unet, [inputs2])
    if a.tiny:
        names = list(quantizable_layers(unet))
        w_cfg, a_cfg = {n: 8 for n in names}, {n: 8 for n in names if n not in ("conv_in", "conv_out")}
    else:
        w_cfg, a_cfg = cfgs.load("weight/uniform_8"), cfgs.load("act/act_8.00")
    quantize_unet(unet, _Cfg(w_cfg, a_cfg), ckpt, bos=True, bos_dict=precompute_bos(unet, inputs2["encoder_hidden_states"]))
    del ckpt
    unet.set_fused(True)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return 1e3 * (time.perf_counter() - t0), out

    def run_case(name, n_steps, B, g):
        sms = {k: Sampler(unet, k, n_steps, guidance_scale=g) for k in ("euler", "dpmpp_2m")}
        rows = sms["euler"].rows_per_image
        inp = example_inputs(B * rows, L, dev, seed=7, cfg=cfg)
        ehs, added = inp["encoder_hidden_states"], inp["added_cond_kwargs"]
        noise = torch.randn(B, 4, L, L, generator=torch.Generator(device="cpu").manual_seed(11)).to(dev)
        ms, outs = {k: [] for k in sms}, {}
        with torch.no_grad():
            for k, sm in sms.items():
                for _ in range(2):
                    sm.sample(noise, ehs, added)
            for _ in range(a.repeats):
                for k, sm in sms.items():
                    dt, outs[k] = timed(lambda: sm.sample(noise, ehs, added))
                    ms[k].append(round(dt, 3))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: round(max(v) - min(v), 3) for k, v in ms.items()}
        diff = round(med["dpmpp_2m"] - med["euler"], 3)
        rec = {"case": name, "n_steps": n_steps, "batch": B, "unet_rows": B * rows, "guidance": g, "ms": ms,
               "median_ms": med, "spread_ms": spread, "dpmpp_2m_minus_euler_ms": diff,
               "per_step_ms": round(diff / n_steps, 4), "within_euler_spread": bool(diff <= spread["euler"]),
               "latents_finite": {k: bool(torch.isfinite(v).all()) for k, v in outs.items()}}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del sms
        torch.cuda.empty_cache()

    tag = "tiny" if a.tiny else "sdxl_1024px"
    run_case(f"{tag}_20step_guided_bs8", 20, 8, 7.5)
    run_case(f"{tag}_4step_bs1", 4, 1, 0.0)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_multistep.py: mixdq_sampler_step_2m vs mixdq_sampler_step (launch pairs, us), and "
                    "Sampler('dpmpp_2m') vs Sampler('euler') whole runs (ms)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
