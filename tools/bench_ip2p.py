"""What InstructPix2Pix costs: the three-row step launch against the two-row one, and a whole Sampler.instruct run against
the same captured UNet with guidance and scheduler step done by eager torch operations between the replays.

    python tools/bench_ip2p.py [--repeats 7] [--out profiles/ip2p_bench.txt]

One box, one process, medians of alternating runs, the spread (max - min) beside every median.
  launch  the step launch pair (the step kernel + the one-thread advance behind it), ROWS 3 (mixdq_sampler_step3) against
          ROWS 2 (mixdq_sampler_step), plain Euler, batch 1 at SD 1.5's 512-px latent size (4 x 64 x 64) and at SDXL's
          1024-px one (4 x 128 x 128): `--launches` launch pairs walking a 1000-step table, captured ONCE into a graph per
          variant and replayed, timed with device events.  ROWS 3 reads one more FP16 row block and writes one more.
  run     Sampler(..., image_guidance_scale=).instruct() on the SD 1.5 UNet with an 8-channel conv_in
          (SD15_IP2P_CONFIG) at 512 px, batch 1 (3 UNet rows), `--steps` Euler steps, uniform W8A8 + BOS with conv_in in
          FP16, synthetic weights, the fused graph (set_fused, as tools/bench_sd15.py's last network), full-size VAE
          encoder and decoder -- against `eager`: the same encode, conditioning and decode, the same UNet forward
          captured into a graph on static buffers, and between the replays the three-row guidance, the Euler update, the
          FP16 input into the three row blocks and the next timestep as eager torch operations fed by Python floats
          (the loop diffusers' pipeline runs; nothing in it waits for the GPU either).  Host clock from the call to a
          device synchronise behind it.
The `run` line says whether the device-side median exceeds the eager median by more than the eager runs' own spread.
This tool measures time only: the weights are synthetic, there is no tokenizer, and no image quality is measured."""
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--tiny", action="store_true", help="the tiny UNet and VAE at latent 32 instead (a rehearsal, not a figure)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ip2p.py needs a GPU"
    import bench
    from mixdq_amd import Sampler, _C
    from mixdq_amd import vae as V
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.sampler import schedule
    from mixdq_amd.unet import SD15_IP2P_CONFIG, build_unet, quantizable_layers
    dev = torch.device("cuda:0")
    G_T, G_I = 7.5, 1.5
    head = {"tool": "bench_ip2p", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
            "hip": torch.version.hip, "lib_csrc_sha16": _lib_sha16(_C), "commit": _commit(), "repeats": a.repeats,
            "launches": a.launches, "steps": a.steps, "guidance": G_T, "image_guidance": G_I}
    lines = [json.dumps(head)]
    print(lines[0], flush=True)

    # ---- the launch pair, replayed from a graph -----------------------------------------------------------------
    def launch_case(name, L):
        n = 4 * L * L
        s = schedule("euler", 1000, "trailing")
        x = torch.randn(n, device=dev)
        eps = torch.randn(3 * n, device=dev).half()
        inp = torch.zeros(3 * n, dtype=torch.float16, device=dev)
        tt, coef = torch.from_numpy(s.t_table).to(dev), torch.from_numpy(s.coef).to(dev)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        t_d = torch.zeros((), device=dev)
        fns = {"rows2": lambda: _C.sampler_step(x, eps, inp, coef, tt, step, t_d, G_T, 2),
               "rows3": lambda: _C.sampler_step3(x, eps, inp, coef, tt, step, t_d, G_T, G_I)}
        graphs = {}
        for k, fn in fns.items():
            step.fill_(1)
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream(dev).wait_stream(side)
            graphs[k] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[k]):
                for _ in range(a.launches):
                    fn()
        us = {k: [] for k in fns}
        for rep in range(a.repeats + 2):                    # the first two trips are untimed
            for k, gr in graphs.items():
                x.normal_()
                step.fill_(1)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                gr.replay()
                e1.record()
                torch.cuda.synchronize(dev)
                assert int(step.item()) == 1 + a.launches
                if rep >= 2:
                    us[k].append(round(1e3 * e0.elapsed_time(e1) / a.launches, 3))
        med = {k: statistics.median(v) for k, v in us.items()}
        rec = {"case": name, "n": n, "us_per_launch_pair": us, "median_us": med,
               "spread_us": {k: round(max(v) - min(v), 3) for k, v in us.items()},
               "rows3_minus_rows2_us": round(med["rows3"] - med["rows2"], 3), "extra_bytes_per_step": 4 * n}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    launch_case("launch_sd15_512px_bs1", 32 if a.tiny else 64)
    launch_case("launch_sdxl_1024px_bs1", 32 if a.tiny else 128)

    # ---- a whole instruct run -----------------------------------------------------------------------------------
    L = 32 if a.tiny else 64
    if a.tiny:
        cfg = dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64, in_channels=8)
        vcfg = dict(V.VAE_SDXL_CONFIG, block_out_channels=(32, 64, 128, 512), layers_per_block=1, norm_num_groups=8)
    else:
        cfg, vcfg = SD15_IP2P_CONFIG, V.VAE_SD15_CONFIG
    unet = build_unet(dev, cfg=cfg)
    inputs2 = example_inputs(2, L, dev, seed=42, cfg=cfg, in_channels=8)
    with torch.no_grad():
        ckpt = calibrate(unet, [inputs2])
    names = list(quantizable_layers(unet))
    # conv_in stays out of the activation config: the split conv_in needs it as a floating-point layer
    quantize_unet(unet, _Cfg({n: 8 for n in names}, {n: 8 for n in names if n not in ("conv_in", "conv_out")}), ckpt,
                  bos=True, bos_dict=precompute_bos(unet, inputs2["encoder_hidden_states"]))
    del ckpt
    unet.set_fused(True)
    enc, dec = V.build_vae_encoder(vcfg, seed=11, device=dev), V.build_vae_decoder(vcfg, seed=11, device=dev)
    B, n_steps = 1, a.steps
    inp3 = example_inputs(3 * B, L, dev, seed=7, cfg=cfg)
    ehs, added = inp3["encoder_hidden_states"], inp3["added_cond_kwargs"]
    gen = torch.Generator(device="cpu").manual_seed(11)
    noise = torch.randn(B, 4, L, L, generator=gen).to(dev)
    image = torch.randint(0, 256, (B, 3, 8 * L, 8 * L), generator=gen, dtype=torch.uint8).to(dev)
    sm = Sampler(unet, "euler", n_steps, G_T, image_guidance_scale=G_I)
    sch = sm.schedule

    # the eager variant: the UNet forward alone in a graph, everything between the replays eager torch
    forward = getattr(unet.forward, "__wrapped__", unet.forward)
    x_in = torch.zeros(3 * B, L, L, 4, dtype=torch.float16, device=dev).permute(0, 3, 1, 2)
    t_in = torch.zeros((), dtype=torch.float32, device=dev)
    term_in = None
    state = {}

    def eager_setup(term):
        nonlocal term_in
        term_in = term.clone()

        def fwd():
            return forward(x_in, t_in, ehs, added, cond_term=term_in)[0]
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.no_grad(), torch.cuda.stream(side):
            for _ in range(2):
                fwd()
        torch.cuda.current_stream(dev).wait_stream(side)
        state["graph"] = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(state["graph"]):
            state["eps"] = fwd()

    coef = [[float(v) for v in row] for row in sch.coef]
    ts = [float(v) for v in sch.t_table]

    def eager_run():
        cond = _C.ip2p_cond(enc.moments(image), 3, 1.0)
        term = unet.cond_term(cond)
        if "graph" not in state:
            eager_setup(term)
        term_in.copy_(term)
        x = noise.float() * sch.init_scale
        first = (x * sch.input_scale0).half()
        for r in range(3):
            x_in[r * B:(r + 1) * B].copy_(first)
        t_in.fill_(ts[0])
        for i in range(n_steps):
            state["graph"].replay()
            e = state["eps"].float()
            e_t, e_i, e_u = e[:B], e[B:2 * B], e[2 * B:]
            eg = e_u + G_T * (e_t - e_i) + G_I * (e_i - e_u)
            x = coef[i][0] * x + coef[i][1] * eg
            nxt = (x * coef[i][3]).half()
            for r in range(3):
                x_in[r * B:(r + 1) * B].copy_(nxt)
            t_in.fill_(ts[i + 1])
        return x, dec.decode(x)

    def device_run():
        return sm.instruct(enc, dec, image, noise, ehs, added)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return 1e3 * (time.perf_counter() - t0), out

    runs = {"device": device_run, "eager": eager_run}
    ms, outs = {k: [] for k in runs}, {}
    with torch.no_grad():
        for k, fn in runs.items():
            for _ in range(2):
                fn()
        for _ in range(a.repeats):
            for k, fn in runs.items():
                dt, outs[k] = timed(fn)
                ms[k].append(round(dt, 3))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: round(max(v) - min(v), 3) for k, v in ms.items()}
    diff = round(med["device"] - med["eager"], 3)
    d = (outs["device"][0] - outs["eager"][0]).abs().max().item()
    rec = {"case": ("tiny" if a.tiny else "sd15_ip2p_512px") + f"_{n_steps}step_bs{B}", "n_steps": n_steps, "batch": B,
           "unet_rows": 3 * B, "ms": ms, "median_ms": med, "spread_ms": spread, "device_minus_eager_ms": diff,
           "per_step_ms": round(diff / n_steps, 4), "device_not_slower_than_eager_spread": bool(diff <= spread["eager"]),
           "latents_max_abs_diff_device_vs_eager": d, "latents_max_abs": outs["eager"][0].abs().max().item(),
           "latents_finite": {k: bool(torch.isfinite(v[0]).all()) for k, v in outs.items()}}
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_ip2p.py: mixdq_sampler_step3 (ROWS 3) vs mixdq_sampler_step (ROWS 2) launch pairs replayed "
                    "from a graph (us), and Sampler.instruct vs the same captured UNet with eager torch guidance + Euler "
                    "step between replays (ms); synthetic weights, no image quality measured\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
