"""What guidance rescale costs: the rescaled step launch group against the plain one, with the per-image combine in the
step kernel's prologue or in a launch of its own, and a whole guided run against the same Sampler without rescale and
against the same captured UNet with diffusers' rescale_noise_cfg as eager torch operations between the replays.

    python tools/bench_rescale.py [--repeats 7] [--out profiles/rescale_bench.txt]

Medians of alternating runs, the spread (max - min) beside every median.
  launch  the step launch group replayed from a graph, timed with device events: `plain` (mixdq_sampler_step /
          mixdq_sampler_step3: step + advance) against `rescaled` (mixdq_sampler_step_rescaled: statistics + step +
          advance, the combine in the step's prologue) and `rescaled_combine_launch` (statistics + one-wave combine +
          step + advance), plain Euler, at SD 1.5's 512-px latent size (4 x 64 x 64) and SDXL's 1024-px one
          (4 x 128 x 128), batch 1 and 8, ROWS 2 and 3: `--launches` groups walking a 1000-step table, captured ONCE per
          variant.  The combine's place is a process-wide knob (MIXDQ_RESCALE_COMBINE_LAUNCH, read once), so the two
          rescaled variants come from child processes of this tool, started in turn (A B A B); `plain` is measured in
          each of them and reported from all.
  run     Sampler(..., guidance_rescale=0.7).sample() on the SD 2.1 UNet (SD21_CONFIG) at 512 px, batch 8 (16 UNet rows),
          `--steps` Euler steps, v-prediction, uniform W8A8 + BOS, synthetic weights, the fused graph -- against `plain`:
          the same Sampler without rescale, and `eager`: the same UNet forward captured into a graph on static buffers,
          and between the replays guidance, rescale_noise_cfg (two torch.std over (1, 2, 3)), the Euler update, the FP16
          input into both row blocks and the next timestep as eager torch operations fed by Python floats.  Host clock
          from the call to a device synchronise behind it.
This tool measures time only: the weights are synthetic, there is no tokenizer, and no image quality is measured."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_sd15 import _commit, _lib_sha16  # noqa: E402

G_T, G_I, PHI = 7.5, 1.5, 0.7
KNOB = "MIXDQ_RESCALE_COMBINE_LAUNCH"


class _Cfg:
    def __init__(self, w, a):
        self.w_config, self.a_config = w, a


def launch_cases(a, dev):
    """[{case, us per launch group: {plain: [...], rescaled: [...]}}] of this process (whatever the knob says)."""
    from mixdq_amd import _C
    from mixdq_amd.sampler import schedule
    out = []
    s = schedule("euler", 1000, "trailing", prediction_type="v_prediction")
    tt, coef = torch.from_numpy(s.t_table).to(dev), torch.from_numpy(s.coef).to(dev)
    for name, L in (("sd15_512px", 32 if a.tiny else 64), ("sdxl_1024px", 32 if a.tiny else 128)):
        for B in (1, 8):
            for rows in (2, 3):
                n_image = 4 * L * L
                n = B * n_image
                x = torch.randn(n, device=dev)
                eps = torch.randn(rows * n, device=dev).half()
                inp = torch.zeros(rows * n, dtype=torch.float16, device=dev)
                ws = _C.sampler_rescale_workspace(n, n_image, dev)
                step = torch.zeros(1, dtype=torch.int32, device=dev)
                t_d = torch.zeros((), device=dev)
                if rows == 2:
                    plain = lambda: _C.sampler_step(x, eps, inp, coef, tt, step, t_d, G_T, 2)      # noqa: E731
                else:
                    plain = lambda: _C.sampler_step3(x, eps, inp, coef, tt, step, t_d, G_T, G_I)    # noqa: E731
                fns = {"plain": plain,
                       "rescaled": lambda: _C.sampler_step_rescaled(x, eps, inp, coef, tt, step, t_d, G_T,
                                                                    G_I if rows == 3 else None, PHI, ws,
                                                                    rows_per_image=rows, n_image=n_image)}
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
                for rep in range(a.repeats + 2):            # the first two trips are untimed
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
                out.append({"case": f"launch_{name}_bs{B}_rows{rows}", "n": n, "us": us})
                del graphs
    return out


def whole_run(a, dev, lines):
    import bench
    from mixdq_amd import Sampler
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import SD21_CONFIG, build_unet, quantizable_layers
    L, B, n_steps = (32 if a.tiny else 64), 8, a.steps
    cfg = dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64) if a.tiny else SD21_CONFIG
    unet = build_unet(dev, cfg=cfg)
    inputs2 = example_inputs(2, L, dev, seed=42, cfg=cfg)
    with torch.no_grad():
        ckpt = calibrate(unet, [inputs2])
    names = list(quantizable_layers(unet))
    quantize_unet(unet, _Cfg({n: 8 for n in names}, {n: 8 for n in names if n not in ("conv_in", "conv_out")}), ckpt,
                  bos=True, bos_dict=precompute_bos(unet, inputs2["encoder_hidden_states"]))
    del ckpt
    unet.set_fused(True)
    inp = example_inputs(2 * B, L, dev, seed=7, cfg=cfg)
    ehs, added = inp["encoder_hidden_states"], inp["added_cond_kwargs"]
    noise = torch.randn(B, 4, L, L, generator=torch.Generator(device="cpu").manual_seed(11)).to(dev)
    kw = dict(prediction_type="v_prediction")
    sm = {"rescaled": Sampler(unet, "euler", n_steps, G_T, guidance_rescale=PHI, **kw),
          "plain": Sampler(unet, "euler", n_steps, G_T, **kw)}
    sch = sm["plain"].schedule
    forward = getattr(unet.forward, "__wrapped__", unet.forward)
    x_in = torch.zeros(2 * B, L, L, 4, dtype=torch.float16, device=dev).permute(0, 3, 1, 2)
    t_in = torch.zeros((), dtype=torch.float32, device=dev)
    state = {}

    def eager_setup():
        def fwd():
            return forward(x_in, t_in, ehs, added)[0]
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
        if "graph" not in state:
            eager_setup()
        x = noise.float() * sch.init_scale
        first = (x * sch.input_scale0).half()
        x_in[:B].copy_(first)
        x_in[B:].copy_(first)
        t_in.fill_(ts[0])
        for i in range(n_steps):
            state["graph"].replay()
            e = state["eps"].float()
            e_u, e_t = e[:B], e[B:]
            eg = e_u + G_T * (e_t - e_u)
            # diffusers' rescale_noise_cfg
            std_text = e_t.std(dim=(1, 2, 3), keepdim=True)
            std_cfg = eg.std(dim=(1, 2, 3), keepdim=True)
            eg = PHI * (eg * (std_text / std_cfg)) + (1 - PHI) * eg
            x = coef[i][0] * x + coef[i][1] * eg
            nxt = (x * coef[i][3]).half()
            x_in[:B].copy_(nxt)
            x_in[B:].copy_(nxt)
            t_in.fill_(ts[i + 1])
        return x

    runs = {"rescaled": lambda: sm["rescaled"].sample(noise, ehs, added),
            "plain": lambda: sm["plain"].sample(noise, ehs, added), "eager": eager_run}

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return 1e3 * (time.perf_counter() - t0), out

    ms, outs = {k: [] for k in runs}, {}
    with torch.no_grad():
        for fn in runs.values():
            for _ in range(2):
                fn()
        for _ in range(a.repeats):
            for k, fn in runs.items():
                dt, outs[k] = timed(fn)
                ms[k].append(round(dt, 3))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: round(max(v) - min(v), 3) for k, v in ms.items()}
    extra = round(med["rescaled"] - med["plain"], 3)
    rec = {"case": ("tiny" if a.tiny else "sd21_512px") + f"_{n_steps}step_bs{B}", "n_steps": n_steps, "batch": B,
           "unet_rows": 2 * B, "ms": ms, "median_ms": med, "spread_ms": spread, "rescaled_minus_plain_ms": extra,
           "per_step_us": round(1e3 * extra / n_steps, 2),
           "added_launches_within_plain_spread": bool(extra <= spread["plain"]),
           "rescaled_minus_eager_ms": round(med["rescaled"] - med["eager"], 3),
           "latents_max_abs_diff_rescaled_vs_eager": (outs["rescaled"] - outs["eager"]).abs().max().item(),
           "latents_max_abs": outs["eager"].abs().max().item(),
           "latents_finite": {k: bool(torch.isfinite(v).all()) for k, v in outs.items()}}
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--tiny", action="store_true", help="small shapes and the tiny UNet (a rehearsal, not a figure)")
    ap.add_argument("--child", action="store_true", help="(internal) print this process's launch cases as JSON")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rescale.py needs a GPU"
    dev = torch.device("cuda:0")
    if a.child:
        print("CHILD " + json.dumps(launch_cases(a, dev)), flush=True)
        return
    from mixdq_amd import _C
    head = {"tool": "bench_rescale", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
            "hip": torch.version.hip, "lib_csrc_sha16": _lib_sha16(_C), "commit": _commit(), "repeats": a.repeats,
            "launches": a.launches, "steps": a.steps, "guidance": G_T, "image_guidance": G_I, "rescale": PHI}
    lines = [json.dumps(head)]
    print(lines[0], flush=True)
    # ---- the launch group: one fresh child per setting of the knob, in turn (this process has not touched the GPU
    # beyond its name: the children run one at a time)
    merged = {}
    for which in ("prologue", "combine_launch") * 2:
        env = {k: v for k, v in os.environ.items() if k != KNOB}
        if which == "combine_launch":
            env[KNOB] = "1"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(a.repeats), "--launches",
               str(a.launches)] + (["--tiny"] if a.tiny else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        got = json.loads(next(l for l in r.stdout.split("\n") if l.startswith("CHILD "))[6:])
        for c in got:
            m = merged.setdefault(c["case"], {"n": c["n"], "plain": [], "rescaled": [], "rescaled_combine_launch": []})
            m["plain"] += c["us"]["plain"]
            m["rescaled" if which == "prologue" else "rescaled_combine_launch"] += c["us"]["rescaled"]
    for case, m in merged.items():
        us = {k: m[k] for k in ("plain", "rescaled", "rescaled_combine_launch")}
        med = {k: statistics.median(v) for k, v in us.items()}
        rec = {"case": case, "n": m["n"], "us_per_launch_group": us, "median_us": med,
               "spread_us": {k: round(max(v) - min(v), 3) for k, v in us.items()},
               "rescaled_minus_plain_us": round(med["rescaled"] - med["plain"], 3),
               "combine_launch_minus_prologue_us": round(med["rescaled_combine_launch"] - med["rescaled"], 3)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    whole_run(a, dev, lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_rescale.py: the rescaled step launch group (statistics + step + advance; the per-image "
                    "combine in the step's prologue, or in a launch of its own) vs the plain one, replayed from a graph "
                    "(us), and a guided Euler run with and without guidance rescale vs the same captured UNet with eager "
                    "torch rescale_noise_cfg between replays (ms); synthetic weights, no image quality measured\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
