"""Latency of whole sampling runs: mixdq_amd.Sampler against the loop a user writes around the UNet without it.

    python tools/bench_sampler.py [--repeats 7] [--out profiles/sampler_bench.txt]

One box, one process, uniform W8A8 + BOS, synthetic weights, the fused graph:
  SDXL UNet at 1024 px (latent 128): 1 and 4 euler_ancestral steps at batch 1; 20 guided euler steps at batch 8 (the
  UNet at 16 rows); SD 1.5 UNet at 512 px (latent 64): 4 lcm steps at batch 1.
Two loops per case, alternating, `--repeats` times each after 2 untimed runs:
  sampler  Sampler.sample(): one captured graph of UNet forward + mixdq_sampler_step, replayed n_steps times.
  eager    the same per-step hipGraph of the UNet forward (hip_graph_opt) with the scheduler and the guidance as
           eager torch operations between the replays: scale the input, cast, (concatenate for guidance), copy the
           timestep, replay, (chunk and combine), a * x + b * e (+ c * n).  Written WITHOUT a host synchronisation
           and with the timesteps already on the device: the favourable form of that loop (diffusers' schedulers
           look their step index up with a host round trip).
A run is timed on the host clock from the call to a device synchronise behind it, inputs already on the device.
Prints one JSON line per case; both loops' latents are compared bit for bit."""
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


def _eager_loop(unet, sch, g, rows, noise, ehs, added, step_noise, consts):
    """The user's loop of today on the graphed UNet: every line below is one or two small eager kernels."""
    t_dev, init_scale = consts
    x = noise.float() * init_scale
    scale = sch.input_scale0
    for i in range(sch.n_steps):
        a, b, c, s_next = (float(v) for v in sch.coef[i])
        inp = (x * scale).half()
        if rows == 2:
            inp = torch.cat([inp, inp])
        eps = unet(inp, t_dev[i], ehs, added)[0].float()
        if rows == 2:
            eu, ec = eps.chunk(2)
            eps = eu + g * (ec - eu)
        x = a * x + b * eps
        if step_noise is not None:
            x = x + c * step_noise[i]
        scale = s_next
    return x


def _timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--tiny", action="store_true", help="the tiny UNet at latent 32 instead (a rehearsal, not a figure)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sampler.py needs a GPU"
    import bench
    from mixdq_amd import Sampler, _C, cfgs
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, hip_graph_opt, quantize_unet
    from mixdq_amd.unet import SD15_CONFIG, build_unet, quantizable_layers
    dev = torch.device("cuda:0")
    head = {"tool": "bench_sampler", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
            "hip": torch.version.hip, "lib_csrc_sha16": _lib_sha16(_C), "commit": _commit(), "repeats": a.repeats,
            "unit": "ms per sample() call, host clock to device synchronise"}
    lines = [json.dumps(head)]
    print(lines[0], flush=True)

    def network(which):
        if a.tiny:
            cfg, L = dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64), 32
        else:
            cfg, L = (SD15_CONFIG, 64) if which == "sd15" else (None, 128)
        unet = build_unet(dev, cfg=cfg)
        inputs2 = example_inputs(2, L, dev, seed=42, cfg=cfg)
        ckpt = calibrate(unet, [inputs2])
        if which == "sdxl" and not a.tiny:
            w_cfg, a_cfg = cfgs.load("weight/uniform_8"), cfgs.load("act/act_8.00")
        else:
            names = list(quantizable_layers(unet))
            w_cfg, a_cfg = {n: 8 for n in names}, {n: 8 for n in names if n not in ("conv_in", "conv_out")}
        quantize_unet(unet, _Cfg(w_cfg, a_cfg), ckpt, bos=True,
                      bos_dict=precompute_bos(unet, inputs2["encoder_hidden_states"]))
        del ckpt
        unet.set_fused(True)
        return unet, cfg, L

    def case(unet, cfg, L, name, kind, n_steps, B, g):
        sm = Sampler(unet, kind, n_steps, guidance_scale=g)
        sch, rows = sm.schedule, sm.rows_per_image
        inp = example_inputs(B * rows, L, dev, seed=7, cfg=cfg)
        ehs, added = inp["encoder_hidden_states"], inp["added_cond_kwargs"]
        gen = torch.Generator(device="cpu").manual_seed(11)
        noise = torch.randn(B, 4, L, L, generator=gen).to(dev)
        sn = torch.randn(n_steps, B, 4, L, L, generator=gen).to(dev) if sch.uses_noise else None
        consts = ([torch.tensor(float(t), device=dev) for t in sch.timesteps],
                  torch.tensor(sch.init_scale, dtype=torch.float32, device=dev))
        eager_forward = unet.forward
        hip_graph_opt(unet)
        graphed = unet.forward
        try:
            loops = {"sampler": lambda: sm.sample(noise, ehs, added, sn),
                     "eager": lambda: _eager_loop(graphed, sch, g, rows, noise, ehs, added, sn, consts)}
            ms, outs = {k: [] for k in loops}, {}
            with torch.no_grad():
                for k, fn in loops.items():
                    for _ in range(2):
                        fn()
                for _ in range(a.repeats):
                    for k, fn in loops.items():
                        dt, outs[k] = _timed(fn, dev)
                        ms[k].append(round(dt, 3))
        finally:
            unet.forward = eager_forward
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec = {"case": name, "kind": kind, "n_steps": n_steps, "batch": B, "unet_rows": B * rows, "guidance": g,
               "ms": ms, "median_ms": med, "min_ms": {k: min(v) for k, v in ms.items()},
               "eager_minus_sampler_ms_per_step": round((med["eager"] - med["sampler"]) / n_steps, 4),
               "sampler_over_eager": round(med["sampler"] / med["eager"], 4),
               "latents_bit_equal": bool(torch.equal(outs["sampler"], outs["eager"])),
               "latents_finite": bool(torch.isfinite(outs["sampler"]).all())}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del sm
        torch.cuda.empty_cache()

    unet, cfg, L = network("sdxl")
    tag = "tiny" if a.tiny else "sdxl_1024px"
    case(unet, cfg, L, f"{tag}_euler_ancestral_1step_bs1", "euler_ancestral", 1, 1, 0.0)
    case(unet, cfg, L, f"{tag}_euler_ancestral_4step_bs1", "euler_ancestral", 4, 1, 0.0)
    case(unet, cfg, L, f"{tag}_euler_20step_guided_bs8", "euler", 20, 8, 7.5)
    del unet
    torch.cuda.empty_cache()
    if not a.tiny:
        unet, cfg, L = network("sd15")
        case(unet, cfg, L, "sd15_512px_lcm_4step_bs1", "lcm", 4, 1, 0.0)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_sampler.py: whole sampling runs, Sampler (one graph: UNet + mixdq_sampler_step) vs the "
                    "eager loop around the same per-step UNet graph\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
