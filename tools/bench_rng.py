"""What noise made on the device costs: the step launch with generated noise against the buffer-fed one, _C.randn against
torch.randn, and whole seeded 'euler_ancestral' runs against the same runs fed a step_noise tensor.

    python tools/bench_rng.py [--repeats 7] [--out profiles/rng_bench.txt]

One box, one process, medians of alternating runs.
  launch  (each also with its `--launches` calls captured into one graph and replayed -- "graphed": back-to-back launches
          from Python are bound by the host's launch rate, a replay by the device)
          the step launch pair (the step kernel + the one-thread advance behind it) at SDXL's latent size (4 x 128 x
          128 per image), batch 1 unguided and batch 8 guided: `--launches` back-to-back launches walking a 1000-step
          'euler_ancestral' table from step 1, noise read from block *step of a [launches + 1, n] buffer (as a
          Sampler's launch reads it: a block no earlier launch touched) against noise computed from seeds, timed with
          device events.
  randn   _C.randn against torch's own generator (Tensor.normal_, what torch.randn runs, into a preallocated tensor) for
          the same [B, 4, 128, 128] FP32 tensor, `--launches` back-to-back calls, device events; _C.randn also graphed
          (torch's generator is left out of that: capturing it needs its state registered with the graph).
  run     Sampler.sample() on the SDXL UNet at 1024 px, uniform W8A8 + BOS, synthetic weights, the fused graph: 4
          'euler_ancestral' steps at batch 1 and at batch 8 guided, `seed=` with a shape against a noise tensor and a
          [4, B, 4, 128, 128] step_noise tensor (made before the clock starts), host clock from the call to a device
          synchronise behind it.
The claim under test: the seeded run is not slower than the tensor-fed run by more than the tensor-fed run's own spread
(max - min); each `run` line says so.  The single launch is expected to turn ALU-bound; it is reported as measured."""
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
    assert torch.cuda.is_available(), "bench_rng.py needs a GPU"
    import bench
    from mixdq_amd import Sampler, _C, cfgs
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.sampler import schedule
    from mixdq_amd.unet import build_unet, quantizable_layers
    dev = torch.device("cuda:0")
    head = {"tool": "bench_rng", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
            "hip": torch.version.hip, "lib_csrc_sha16": _lib_sha16(_C), "commit": _commit(), "repeats": a.repeats,
            "launches": a.launches}
    lines = [json.dumps(head)]
    print(lines[0], flush=True)
    L = 32 if a.tiny else 128
    n_image = 4 * L * L

    def graphed(fns):
        """Each fn's `--launches` calls captured into one graph: a replay is bound by the device, not by the host's
        launch rate."""
        out = {}
        for k, fn in fns.items():
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream(dev).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(a.launches):
                    fn()
            out[k] = graph
        return out

    def event_us(fns, before, graphs=None):
        us = {k: [] for k in fns}
        for rep in range(a.repeats + 2):                    # the first two trips are untimed
            for k, fn in fns.items():
                before()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if graphs is None:
                    for _ in range(a.launches):
                        fn()
                else:
                    graphs[k].replay()
                e1.record()
                torch.cuda.synchronize(dev)
                if rep >= 2:
                    us[k].append(round(1e3 * e0.elapsed_time(e1) / a.launches, 3))
        return us

    # ---- the launch pair ----------------------------------------------------------------------------------------
    def launch_case(B, rows, g):
        n = B * n_image
        s = schedule("euler_ancestral", 1000)
        assert (s.coef[:a.launches + 1, 2] != 0).all()
        x = torch.randn(n, device=dev)
        eps = torch.randn(rows * n, device=dev).half()
        inp = torch.zeros(rows * n, dtype=torch.float16, device=dev)
        tt, coef = torch.from_numpy(s.t_table).to(dev), torch.from_numpy(s.coef).to(dev)
        step, t_d = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((), device=dev)
        # the buffer-fed launch reads block *step of a [launches + 1, n] buffer, as a Sampler's does
        noise = torch.randn((a.launches + 1) * n, device=dev)
        seeds = torch.arange(1, B + 1, dtype=torch.int64, device=dev)
        fns = {"buffer": lambda: _C.sampler_step(x, eps, inp, coef[:a.launches + 1], tt, step, t_d, g, rows, noise),
               "rng": lambda: _C.sampler_step(x, eps, inp, coef, tt, step, t_d, g, rows, seeds=seeds, n_image=n_image)}

        def before():
            x.normal_()
            step.fill_(1)
        us = event_us(fns, before)
        assert int(step.item()) == 1 + a.launches
        before()
        us_g = event_us(fns, before, graphed(fns))
        assert int(step.item()) == 1 + a.launches
        med = {k: statistics.median(v) for k, v in us.items()}
        med_g = {k: statistics.median(v) for k, v in us_g.items()}
        rec = {"case": f"launch_bs{B}_rows{rows}", "n": n, "us_per_launch_pair": us, "median_us": med,
               "spread_us": {k: round(max(v) - min(v), 3) for k, v in us.items()},
               "rng_minus_buffer_us": round(med["rng"] - med["buffer"], 3),
               "graphed_us_per_launch_pair": us_g, "graphed_median_us": med_g,
               "graphed_rng_minus_buffer_us": round(med_g["rng"] - med_g["buffer"], 3),
               "noise_bytes_not_read_per_step": 4 * n}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    launch_case(1, 1, 0.0)
    launch_case(8, 2, 7.5)

    # ---- randn --------------------------------------------------------------------------------------------------
    def randn_case(B):
        shape = (B, 4, L, L)
        seeds = torch.arange(1, B + 1, dtype=torch.int64, device=dev)
        out = torch.empty((B, L, L, 4), device=dev).permute(0, 3, 1, 2)
        out_t = torch.empty(shape, device=dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        fns = {"torch.randn": lambda: out_t.normal_(generator=gen),
               "_C.randn": lambda: _C.randn(shape, seeds, out=out)}
        us = event_us(fns, lambda: None)
        us_g = event_us({"_C.randn": fns["_C.randn"]}, lambda: None, graphed({"_C.randn": fns["_C.randn"]}))
        med = {k: statistics.median(v) for k, v in us.items()}
        rec = {"case": f"randn_bs{B}", "elements": B * n_image, "us_per_call": us, "median_us": med,
               "spread_us": {k: round(max(v) - min(v), 3) for k, v in us.items()},
               "ours_minus_torch_us": round(med["_C.randn"] - med["torch.randn"], 3),
               "graphed_us_per_call": us_g, "graphed_median_us": statistics.median(us_g["_C.randn"])}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    randn_case(1)
    randn_case(8)

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
        sms = {k: Sampler(unet, "euler_ancestral", n_steps, guidance_scale=g) for k in ("tensor", "seed")}
        rows = sms["seed"].rows_per_image
        inp = example_inputs(B * rows, L, dev, seed=7, cfg=cfg)
        ehs, added = inp["encoder_hidden_states"], inp["added_cond_kwargs"]
        shape = (B, 4, L, L)
        seeds = torch.arange(11, 11 + B, dtype=torch.int64, device=dev)
        noise = _C.randn(shape, seeds)
        sn = torch.stack([_C.randn(shape, seeds, _C.RNG_STREAM_STEP, i) for i in range(n_steps)])
        calls = {"tensor": lambda: sms["tensor"].sample(noise, ehs, added, sn),
                 "seed": lambda: sms["seed"].sample(shape, ehs, added, seed=seeds)}
        ms, outs = {k: [] for k in sms}, {}
        with torch.no_grad():
            for k in sms:
                for _ in range(2):
                    calls[k]()
            for _ in range(a.repeats):
                for k in sms:
                    dt, outs[k] = timed(calls[k])
                    ms[k].append(round(dt, 3))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: round(max(v) - min(v), 3) for k, v in ms.items()}
        diff = round(med["seed"] - med["tensor"], 3)
        rec = {"case": name, "n_steps": n_steps, "batch": B, "unet_rows": B * rows, "guidance": g, "ms": ms,
               "median_ms": med, "spread_ms": spread, "seed_minus_tensor_ms": diff,
               "within_tensor_spread": bool(diff <= spread["tensor"]),
               "same_latents": bool(torch.equal(outs["seed"], outs["tensor"])),
               "step_noise_buffer_bytes": {"tensor": 4 * n_steps * B * n_image, "seed": 0}}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del sms
        torch.cuda.empty_cache()

    tag = "tiny" if a.tiny else "sdxl_1024px"
    run_case(f"{tag}_4step_bs1", 4, 1, 0.0)
    run_case(f"{tag}_4step_guided_bs8", 4, 8, 7.5)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_rng.py: mixdq_sampler_step_rng vs mixdq_sampler_step with a noise buffer (launch pairs, us), "
                    "_C.randn vs torch.randn (us), and Sampler.sample(seed=) vs a step_noise tensor, whole runs (ms)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
