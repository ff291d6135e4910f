"""What the ControlNet glue costs: the one-launch scaled residual add against the torch chain it replaces, the hint
term, and one guided UNet step with a ControlNet against the same step with the scaling as eager torch operations and
against the step without a ControlNet.

    python tools/bench_controlnet.py [--repeats 7] [--out profiles/controlnet_bench.txt]

Medians of alternating runs, the spread (max - min) beside every median.
  add    mixdq_control_add_f16 (ONE launch over every skip tensor and the mid-block output) replayed from a graph, timed
         with device events, against `torch`: per segment K half multiplications by a Python float, K - 1 half additions
         and the addition to the skip, captured into a graph as well -- at the skip sizes of SD 1.5 at 512 px (12 skips +
         mid, latent 64) and of SDXL at 1024 px (9 skips + mid, latent 128), 1 and 2 UNet rows (batch 1, and batch 1
         guided), K = 1 and 2, and `closed`: the same launch with every scale 0 (the residuals are not loaded; dst = skip)
  hint   ControlNet.hint_term (ingest, eight convs, seven SiLU launches) at 512 and 1024 px, one image, host clock
         around a synchronised call
  step   SD15_CONFIG + CONTROLNET_SD15_CONFIG at 512 px, 2 rows, uniform W8A8 + BOS, synthetic weights, the fused graph:
         `control` = ControlNet forward + UNet(control=) captured as ONE graph; `eager_scale` = the ControlNet forward
         captured, then K = 1 multiplication per residual as eager torch operations, then the UNet with diffusers'
         keywords captured; `plain` = the UNet alone, captured.
  run    the same two networks, batch 1 guided (2 rows), `--steps` euler steps: Sampler(controlnet=).sample(control=image)
         against `eager`: the same ControlNet and UNet forwards captured into two graphs on static buffers, and between
         the replays the scaling of the 13 residuals, the guidance, the Euler update, the FP16 input into both row blocks
         and the next timestep as eager torch operations fed by Python floats; and against `plain`: the Sampler without
         a ControlNet.  Host clock from the call to a device synchronise behind it.
This tool measures time only: the weights are synthetic, and no image quality is measured."""
import argparse
import json
import os
import statistics
import sys
import time
import traceback

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_sd15 import _commit, _lib_sha16  # noqa: E402


class _Cfg:
    def __init__(self, w, a):
        self.w_config, self.a_config = w, a


def skip_shapes(cfg, B, L):
    boc, n = cfg["block_out_channels"], cfg["layers_per_block"]
    shapes = [(B, boc[0], L, L)]
    for i, c in enumerate(boc):
        shapes += [(B, c, L, L)] * n
        if i < len(boc) - 1:
            L //= 2
            shapes.append((B, c, L, L))
    return shapes + [(B, boc[-1], L, L)]


def _capture(fn, dev, launches):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    return g


def _alternate(graphs, dev, repeats, per):
    us = {k: [] for k in graphs}
    for rep in range(repeats + 2):                  # the first two trips are untimed
        for k, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize(dev)
            if rep >= 2:
                us[k].append(round(1e3 * e0.elapsed_time(e1) / per, 3))
    return us


def _summary(us):
    return ({k: statistics.median(v) for k, v in us.items()}, {k: round(max(v) - min(v), 3) for k, v in us.items()})


def add_cases(a, dev, lines):
    from mixdq_amd import _C
    from mixdq_amd.unet import SD15_CONFIG, SDXL_CONFIG
    cl = torch.channels_last
    for name, cfg, L in (("sd15_512px", SD15_CONFIG, 16 if a.tiny else 64), ("sdxl_1024px", SDXL_CONFIG, 16 if a.tiny else 128)):
        for rows in (1, 2):
            shapes = skip_shapes(cfg, rows, L)
            skips = [torch.randn(s, device=dev).half().contiguous(memory_format=cl) for s in shapes]
            for K in (1, 2):
                res = [[torch.randn(s, device=dev).half().contiguous(memory_format=cl) for s in shapes] for _ in range(K)]
                scales = [0.75, 1.25][:K]
                table = torch.tensor([[s] for s in scales], device=dev)
                zeros = torch.zeros_like(table)
                step = torch.zeros(1, dtype=torch.int32, device=dev)
                out = [torch.empty_like(s) for s in skips]

                def chain():
                    o = []
                    for i, s in enumerate(skips):
                        acc = res[0][i] * scales[0]
                        for k in range(1, K):
                            acc = acc + res[k][i] * scales[k]
                        o.append(s + acc)
                    return o

                fns = {"control_add": lambda: _C.control_add(skips, res, table, step, out=out),
                       "closed": lambda: _C.control_add(skips, res, zeros, step, out=out),
                       "torch": chain}
                graphs = {k: _capture(fn, dev, a.launches) for k, fn in fns.items()}
                us = _alternate(graphs, dev, a.repeats, a.launches)
                med, spread = _summary(us)
                elems = sum(s.numel() for s in skips)
                rec = {"case": f"add_{name}_rows{rows}_k{K}", "segments": len(skips), "elements": elems,
                       "bytes_moved_control_add": 2 * elems * (2 + K), "us": us, "median_us": med, "spread_us": spread,
                       "torch_over_control_add": round(med["torch"] / med["control_add"], 2),
                       "control_add_gb_per_s": round(2e-3 * elems * (2 + K) / med["control_add"], 1)}
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
                del graphs


def hint_cases(a, dev, lines):
    import bench
    from mixdq_amd.controlnet import CONTROLNET_SD15_CONFIG, build_controlnet
    tiny = dict(bench.TINY_CFG, conditioning_embedding_out_channels=(8, 16, 32, 64))
    net = build_controlnet(dev, cfg=tiny if a.tiny else CONTROLNET_SD15_CONFIG)
    for px in ((64, 128) if a.tiny else (512, 1024)):
        image = torch.randint(0, 256, (1, 3, px, px), dtype=torch.uint8, device=dev)
        for _ in range(3):
            net.hint_term(image)
        ms = []
        for _ in range(a.repeats):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            net.hint_term(image)
            torch.cuda.synchronize(dev)
            ms.append(round(1e3 * (time.perf_counter() - t0), 3))
        lines.append(json.dumps({"case": f"hint_term_{px}px", "ms": ms, "median_ms": statistics.median(ms),
                                 "spread_ms": round(max(ms) - min(ms), 3)}))
        print(lines[-1], flush=True)


def step_case(a, dev, lines):
    import bench
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.controlnet import CONTROLNET_SD15_CONFIG, build_controlnet
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import SD15_CONFIG, ControlResiduals, build_unet, quantizable_layers
    L = 32 if a.tiny else 64
    cfg = dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64) if a.tiny else SD15_CONFIG
    ccfg = dict(cfg, conditioning_embedding_out_channels=CONTROLNET_SD15_CONFIG["conditioning_embedding_out_channels"])
    inp = example_inputs(2, L, dev, seed=42, cfg=cfg)
    image = torch.randint(0, 256, (2, 3, 8 * L, 8 * L), dtype=torch.uint8, device=dev)
    fp16 = ("conv_in", "conv_out", "controlnet_cond_embedding", "controlnet_down_blocks", "controlnet_mid_block")

    def w8a8(net, batch):
        with torch.no_grad():
            ckpt = calibrate(net, [batch])
        names = list(quantizable_layers(net))
        quantize_unet(net, _Cfg({n: 8 for n in names}, {n: 8 for n in names if n.split(".")[0] not in fp16}), ckpt,
                      bos=True, bos_dict=precompute_bos(net, batch["encoder_hidden_states"]))
        return net.set_fused(True)

    unet = w8a8(build_unet(dev, cfg=cfg), inp)
    net = w8a8(build_controlnet(dev, cfg=ccfg), dict(inp, controlnet_cond=image))
    args = (inp["sample"], inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"])
    table = torch.tensor([[0.75]], device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.no_grad():
        term = net.hint_term(image)
        for _ in range(2):                              # (plans, caches)
            down, mid = net(*args, hint_term=term)
            unet(*args, control=ControlResiduals([(down, mid)], table, step))
            unet(*args, down_block_additional_residuals=down, mid_block_additional_residual=mid)
            unet(*args)
        state = {}

        def control():
            d, m = net(*args, hint_term=term)
            return unet(*args, control=ControlResiduals([(d, m)], table, step))[0]

        def only_net():
            state["res"] = net(*args, hint_term=term)

        g_control = _capture(control, dev, 1)
        g_net = _capture(only_net, dev, 1)
        d0, m0 = state["res"]
        scaled = [torch.empty_like(d) for d in d0] + [torch.empty_like(m0)]
        g_unet_kw = _capture(lambda: unet(*args, down_block_additional_residuals=scaled[:-1],
                                          mid_block_additional_residual=scaled[-1]), dev, 1)
        g_plain = _capture(lambda: unet(*args), dev, 1)

        def eager_scale():
            g_net.replay()
            for o, r in zip(scaled, list(d0) + [m0]):
                torch.mul(r, 0.75, out=o)
            g_unet_kw.replay()

        runs = {"control": g_control.replay, "eager_scale": eager_scale, "plain": g_plain.replay}
        ms = {k: [] for k in runs}
        for rep in range(a.repeats + 2):
            for k, fn in runs.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize(dev)
                if rep >= 2:
                    ms[k].append(round(1e3 * (time.perf_counter() - t0) / a.steps, 4))
    med, spread = _summary(ms)
    lines.append(json.dumps({"case": ("tiny" if a.tiny else "sd15_512px") + "_step_rows2", "steps_per_sample": a.steps,
                             "ms_per_step": ms, "median_ms": med, "spread_ms": spread,
                             "control_minus_plain_ms": round(med["control"] - med["plain"], 4),
                             "control_minus_eager_scale_ms": round(med["control"] - med["eager_scale"], 4)}))
    print(lines[-1], flush=True)


def run_case(a, dev, lines):
    """A whole guided `euler` run: Sampler(controlnet=) against the same captured ControlNet and UNet forwards with the
    scaled adds, the guidance and the Euler update as eager torch operations between the replays, and against the
    Sampler without a ControlNet."""
    import bench
    from mixdq_amd import Sampler
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.controlnet import CONTROLNET_SD15_CONFIG, build_controlnet
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import SD15_CONFIG, build_unet, quantizable_layers
    L, B, n_steps, G, SCALE = (32 if a.tiny else 64), 1, a.steps, 7.5, 0.75
    cfg = dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64) if a.tiny else SD15_CONFIG
    ccfg = dict(cfg, conditioning_embedding_out_channels=CONTROLNET_SD15_CONFIG["conditioning_embedding_out_channels"])
    inp = example_inputs(2 * B, L, dev, seed=42, cfg=cfg)
    ehs, added = inp["encoder_hidden_states"], inp["added_cond_kwargs"]
    image = torch.randint(0, 256, (B, 3, 8 * L, 8 * L), dtype=torch.uint8, device=dev)
    fp16 = ("conv_in", "conv_out", "controlnet_cond_embedding", "controlnet_down_blocks", "controlnet_mid_block")

    def w8a8(net, batch):
        with torch.no_grad():
            ckpt = calibrate(net, [batch])
        names = list(quantizable_layers(net))
        quantize_unet(net, _Cfg({n: 8 for n in names}, {n: 8 for n in names if n.split(".")[0] not in fp16}), ckpt,
                      bos=True, bos_dict=precompute_bos(net, batch["encoder_hidden_states"]))
        return net.set_fused(True)

    unet = w8a8(build_unet(dev, cfg=cfg), inp)
    net = w8a8(build_controlnet(dev, cfg=ccfg), dict(inp, controlnet_cond=torch.cat([image] * 2)))
    noise = torch.randn(B, 4, L, L, generator=torch.Generator(device="cpu").manual_seed(11)).to(dev)
    sm = {"control": Sampler(unet, "euler", n_steps, G, controlnet=net), "plain": Sampler(unet, "euler", n_steps, G)}
    sch = sm["plain"].schedule
    x_in = torch.zeros(2 * B, L, L, 4, dtype=torch.float16, device=dev).permute(0, 3, 1, 2)
    t_in = torch.zeros((), dtype=torch.float32, device=dev)
    state = {}

    def eager_setup():
        # (kept in `state`: the graph reads it at every replay, long after this function has returned)
        term = state["term"] = torch.cat([net.hint_term(image)] * 2).contiguous(memory_format=torch.channels_last)

        def net_fwd():
            state["res"] = net(x_in, t_in, ehs, added, hint_term=term)
        g_net = _capture(net_fwd, dev, 1)
        d0, m0 = state["res"]
        state["raw"] = list(d0) + [m0]
        state["scaled"] = [torch.empty_like(r) for r in state["raw"]]

        def unet_fwd():
            state["eps"] = unet(x_in, t_in, ehs, added, down_block_additional_residuals=state["scaled"][:-1],
                                mid_block_additional_residual=state["scaled"][-1])[0]
        state["g_net"], state["g_unet"] = g_net, _capture(unet_fwd, dev, 1)

    coef = [[float(v) for v in row] for row in sch.coef]
    ts = [float(v) for v in sch.t_table]

    def eager_run():
        if "g_net" not in state:
            eager_setup()
        x = noise.float() * sch.init_scale
        first = (x * sch.input_scale0).half()
        x_in[:B].copy_(first)
        x_in[B:].copy_(first)
        t_in.fill_(ts[0])
        for i in range(n_steps):
            state["g_net"].replay()
            for o, r in zip(state["scaled"], state["raw"]):
                torch.mul(r, SCALE, out=o)
            state["g_unet"].replay()
            e = state["eps"].float()
            eg = e[:B] + G * (e[B:] - e[:B])
            x = coef[i][0] * x + coef[i][1] * eg
            nxt = (x * coef[i][3]).half()
            x_in[:B].copy_(nxt)
            x_in[B:].copy_(nxt)
            t_in.fill_(ts[i + 1])
        return x

    runs = {"control": lambda: sm["control"].sample(noise, ehs, added, control=image, control_scale=SCALE),
            "eager": eager_run, "plain": lambda: sm["plain"].sample(noise, ehs, added)}
    ms, outs = {k: [] for k in runs}, {}
    with torch.no_grad():
        for fn in runs.values():
            for _ in range(2):
                fn()
        for _ in range(a.repeats):
            for k, fn in runs.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                outs[k] = fn()
                torch.cuda.synchronize(dev)
                ms[k].append(round(1e3 * (time.perf_counter() - t0), 3))
    # does every variant return the same bits when it is run again? (a difference between two variants means nothing
    # unless each of them is repeatable)
    with torch.no_grad():
        repeatable = {k: bool(torch.equal(fn(), fn())) for k, fn in runs.items()}
        term = torch.cat([net.hint_term(image)] * 2).contiguous(memory_format=torch.channels_last)
        repeatable["hint_term"] = bool(torch.equal(term[:B], net.hint_term(image)))
        r1, r2 = (net(x_in, t_in, ehs, added, hint_term=term) for _ in range(2))
        repeatable["controlnet_forward"] = all(torch.equal(p, q) for p, q in zip(r1[0] + [r1[1]], r2[0] + [r2[1]]))
        u1, u2 = (unet(x_in, t_in, ehs, added, down_block_additional_residuals=r1[0],
                       mid_block_additional_residual=r1[1])[0] for _ in range(2))
        repeatable["unet_with_residuals"] = bool(torch.equal(u1, u2))
        p1, p2 = (unet(x_in, t_in, ehs, added)[0] for _ in range(2))
        repeatable["unet_plain"] = bool(torch.equal(p1, p2))
        # the first step written out without any graph, with the residuals through either entry of the UNet
        from mixdq_amd.unet import ControlResiduals

        def first_step(entry):
            x = noise.float() * sch.init_scale
            first = (x * sch.input_scale0).half()
            x_in[:B].copy_(first)
            x_in[B:].copy_(first)
            t_in.fill_(ts[0])
            d, m = net(x_in, t_in, ehs, added, hint_term=term)
            if entry == "keywords":
                e = unet(x_in, t_in, ehs, added, down_block_additional_residuals=[r * SCALE for r in d],
                         mid_block_additional_residual=m * SCALE)[0].float()
            else:
                ctl = ControlResiduals([(d, m)], torch.full((1, n_steps), SCALE, device=dev),
                                       torch.zeros(1, dtype=torch.int32, device=dev))
                e = unet(x_in, t_in, ehs, added, control=ctl)[0].float()
            return coef[0][0] * x + coef[0][1] * (e[:B] + G * (e[B:] - e[:B]))
        one = {}
        if n_steps == 1:
            ek, ec = first_step("keywords"), first_step("control")
            one = {"keywords_vs_control": (ek - ec).abs().max().item(), "sampler_vs_control": (outs["control"] - ec).abs().max().item(),
                   "graphs_vs_keywords": (outs["eager"] - ek).abs().max().item()}
    med, spread = _summary(ms)
    lines.append(json.dumps({"case": ("tiny" if a.tiny else "sd15_512px") + f"_{n_steps}step_euler_guided_bs{B}",
                             "repeatable": repeatable, "first_step_without_graphs": one,
                             "n_steps": n_steps, "unet_rows": 2 * B, "control_scale": SCALE, "ms": ms, "median_ms": med,
                             "spread_ms": spread, "control_minus_plain_ms": round(med["control"] - med["plain"], 3),
                             "control_minus_eager_ms": round(med["control"] - med["eager"], 3),
                             "latents_max_abs_diff_control_vs_eager": (outs["control"] - outs["eager"]).abs().max().item(),
                             "latents_max_abs": outs["eager"].abs().max().item(),
                             "latents_finite": {k: bool(torch.isfinite(v).all()) for k, v in outs.items()}}))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--tiny", action="store_true", help="small shapes and the tiny networks (a rehearsal, not a figure)")
    ap.add_argument("--skip-step", action="store_true", help="leave the whole-step comparison out")
    ap.add_argument("--only-step", action="store_true", help="the whole-step comparison alone")
    ap.add_argument("--only-run", action="store_true", help="the whole-run comparison alone")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_controlnet.py needs a GPU"
    dev = torch.device("cuda:0")
    from mixdq_amd import _C
    head = {"tool": "bench_controlnet", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
            "hip": torch.version.hip, "lib_csrc_sha16": _lib_sha16(_C), "commit": _commit(), "repeats": a.repeats,
            "launches": a.launches, "steps": a.steps, "control_chunk": _C.CONTROL_CHUNK}
    lines = [json.dumps(head)]
    print(lines[0], flush=True)
    parts = [add_cases, hint_cases, step_case, run_case]
    if a.only_step or a.only_run:
        parts = [step_case] if a.only_step else [run_case]
    elif a.skip_step:
        parts = [add_cases, hint_cases]
    for part in parts:
        try:
            part(a, dev, lines)
        except Exception:                                   # (a part that fails does not take the others' figures along)
            lines.append(json.dumps({"case": part.__name__, "error": traceback.format_exc()[-1500:]}))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_controlnet.py: mixdq_control_add_f16 vs the torch chain it replaces, both replayed from a "
                    "graph (us per launch / chain); ControlNet.hint_term (ms); one guided SD 1.5 UNet step at 512 px with a "
                    "ControlNet, as one graph vs with the scaling as eager torch operations vs without a ControlNet (ms); a "
                    "whole guided euler run, Sampler(controlnet=) vs the same captured forwards with eager torch operations "
                    "between them vs the Sampler without a ControlNet (ms); synthetic weights, no image quality measured.  "
                    "`lib_csrc_sha16` identifies the kernel sources measured; `commit` is \"unknown\" where the tool ran "
                    "from a copy of the tree without git metadata\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
