#!/usr/bin/env python3
"""The SDXL step with packed-W4 3x3 convs on the LDS-halo kernel against the same step with those convs on the
implicit-GEMM family (MIXDQ_HALO_W4=0), on one MI355X.

weight_4.00 + act_7.77, w4_kernel=True, 1024 px, fused graph, hipGraph replay.  The switch is read once per process,
so each setting lives in a child process of its own (this script with --child): it builds the network, captures the
graph and then replays it `iters` times whenever the parent writes a line to its stdin, answering with the ms per
replay.  The parent alternates the two children over `rounds` rounds (tools/bench_w2.py's A/B) and prints medians,
the spread of each series, the conv launches of a step by kernel family and the peak dynamic memory of a step.
(Each child calibrates for itself with stock FP16 ops, whose bits differ from process to process, so the outputs of
the two children are not compared here: `bench.py --dump-outputs` does that with its deterministic calibration.)

    python tools/bench_halo_w4.py [--batch 1] [--rounds 10] [--iters 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def child(batch, iters):
    import torch
    from mixdq_amd import _C as C
    from mixdq_amd import cfgs
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet

    class Args:
        w_config, a_config = cfgs.load("weight/weight_4.00"), cfgs.load("act/act_7.77")
    unet = build_unet(DEV)
    calib_in = example_inputs(2, 128, DEV, seed=7)
    ckpt = calibrate(unet, [calib_in])
    bos = precompute_bos(unet, calib_in["encoder_hidden_states"])
    quantize_unet(unet, Args, ckpt, bos=True, bos_dict=bos, w4_kernel=True)
    del ckpt, calib_in
    unet.set_fused(True)
    inputs = example_inputs(batch, 128, DEV, seed=0)
    C.RECORD = []
    folds, real = [0], C.qconv2d_w8_a8_ohalf

    def counting(*args, **kw):
        folds[0] += bool(kw.get("_upsample2x"))
        return real(*args, **kw)
    C.qconv2d_w8_a8_ohalf = counting
    with torch.no_grad():
        unet(**inputs)
    kinds = [e[0] for e in C.RECORD]
    C.RECORD, C.qconv2d_w8_a8_ohalf = None, real
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(2):
            unet(**inputs)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        unet(**inputs)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        unet(**inputs)
    g.replay()
    torch.cuda.synchronize()
    info = dict(ready=True, halo_w4=os.environ.get("MIXDQ_HALO_W4", "1"), launches_recorded=len(kinds),
                conv_halo_launches=sum(k.startswith("conv_halo") for k in kinds),
                conv_igemm_launches=sum(k == "conv" for k in kinds), upsample_folds=folds[0], peak_dynamic_mb=round(peak / 2 ** 20, 1))
    print(json.dumps(info), flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        print(json.dumps(dict(ms=a.elapsed_time(b) / iters)), flush=True)


def _read(p):
    while True:
        line = p.stdout.readline()
        if not line:
            raise SystemExit(f"a child ended early (exit {p.wait()})")
        if line.startswith("{"):
            return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.batch, a.iters)
    procs = {}
    for name, flag in (("halo", "1"), ("igemm", "0")):
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--batch", str(a.batch),
                                        "--iters", str(a.iters)], env=dict(os.environ, MIXDQ_HALO_W4=flag),
                                       stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=ROOT)
    try:
        info = {k: _read(p) for k, p in procs.items()}
        ms = {k: [] for k in procs}
        for _ in range(a.rounds):
            for k, p in procs.items():
                p.stdin.write("go\n")
                p.stdin.flush()
                ms[k].append(_read(p)["ms"])
    finally:
        for p in procs.values():
            try:
                p.stdin.close()
            except OSError:
                pass
        for p in procs.values():
            p.wait(timeout=120)
    res = dict(batch=a.batch, rounds=a.rounds, iters=a.iters,
               step_ms={k: round(statistics.median(v), 3) for k, v in ms.items()},
               spread_ms={k: round(max(v) - min(v), 3) for k, v in ms.items()},
               step_ms_all={k: [round(x, 3) for x in v] for k, v in ms.items()}, children=info)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
