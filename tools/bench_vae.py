"""Latency of the FP16 VAE decoder (mixdq_amd.vae) next to the same network on stock PyTorch, same box, same process.

    python tools/bench_vae.py [--repeats 7] [--out profiles/vae_bench.txt] [--no-kernel-stats]

Synthetic weights (build_vae_decoder, seed 42) -- every number below is with them.  Cases: SDXL 1024 px (latents
128 x 128) at batch 1 and 4, SD 1.5 512 px (latents 64 x 64) at batch 1.  Per case:
  ours    hipGraph replays of VAEDecoder.decode (hip_graph_opt)
  stock   the decoder of tests/vae_ref.py (nn.Conv2d / nn.GroupNorm / F.interpolate / SDPA) in FP16, channels-last,
          under the same capture where the stock operators can be captured, else eager (the line says which)
alternating, `--repeats` timed runs each after 2 untimed ones; a run is timed on the host clock from the call to a
device synchronise behind it.  Reported: median and [min, max].
Before the timing, one full-size smoke: the 1024-px decode is finite everywhere and launches no kernel that is not
this library's, apart from the conversion of the 4-channel input (torch.profiler).
Last, unless --no-kernel-stats: one child process under `rocprofv3 --kernel-trace --stats` runs ten eager 1024-px
decodes; the per-kernel table is appended.
"""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def _timed(fn):
    torch.cuda.synchronize(DEV)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(DEV)
    return 1e3 * (time.perf_counter() - t0)


def _latents(cfg, B, L, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(B, 4, L, L, generator=g) * cfg["scaling_factor"]).to(DEV)


def kernel_audit(vae, z):
    """Names of the device kernels of one eager decode, split into this library's and the rest."""
    from torch.profiler import ProfilerActivity, profile
    vae.decode(z)
    torch.cuda.synchronize(DEV)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        vae.decode(z)
        torch.cuda.synchronize(DEV)
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
             and "Memcpy" not in e.name and "Memset" not in e.name]
    return [n for n in names if "mixdq" in n], [n for n in names if "mixdq" not in n]


def smoke(vae, cfg, say):
    z = _latents(cfg, 1, 128)
    img = vae.decode(z)
    torch.cuda.synchronize(DEV)
    finite = bool(torch.isfinite(img).all())
    ours, other = kernel_audit(vae, z)
    say(json.dumps(dict(smoke="1024 px decode", shape=list(img.shape), finite=finite, abs_max=float(img.float().abs().max()),
                        library_kernels=len(ours), other_kernels=other)))
    if not finite:
        raise SystemExit("bench_vae: the 1024-px decode is not finite")
    if ours and (len(other) > 2 or not all("copy" in n.lower() or "elementwise" in n.lower() for n in other)):
        raise SystemExit("bench_vae: a decode launches kernels that are not this library's: %r" % other)


def one_decode_loop(n):
    from mixdq_amd import vae as V
    vae = V.build_vae_decoder(V.VAE_SDXL_CONFIG, device=DEV)
    z = _latents(V.VAE_SDXL_CONFIG, 1, 128)
    for _ in range(n):
        vae.decode(z)
    torch.cuda.synchronize(DEV)


def kernel_stats(say):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--decode-loop", "10"]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            say("kernel stats: rocprofv3 run failed (exit %d)\n%s" % (r.returncode, r.stdout[-1500:]))
            return
        say("per-kernel statistics of ten eager 1024-px decodes, batch 1 (rocprofv3 --kernel-trace --stats), by total time:")
        say("  %-8s %10s %10s %7s  %s" % ("calls", "total ms", "avg us", "%", "kernel"))
        import csv
        with open(files[0], newline="") as f:
            for i, row in enumerate(csv.DictReader(f)):
                if i < 24:
                    say("  %-8s %10.3f %10.1f %7.2f  %s" % (row["Calls"], float(row["TotalDurationNs"]) / 1e6,
                                                          float(row["AverageNs"]) / 1e3, float(row["Percentage"]),
                                                          row["Name"][:150]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-kernel-stats", action="store_true")
    ap.add_argument("--no-stock", action="store_true")
    ap.add_argument("--decode-loop", type=int, default=0, help="(child of the rocprofv3 run) eager 1024-px decodes")
    args = ap.parse_args()
    if args.decode_loop:
        return one_decode_loop(args.decode_loop)
    from mixdq_amd import vae as V
    from mixdq_amd.quantize_sdxl import hip_graph_opt
    from tests import vae_ref
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# tools/bench_vae.py -- synthetic weights; %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    cases = [("sdxl_1024", V.VAE_SDXL_CONFIG, 128, 1), ("sdxl_1024", V.VAE_SDXL_CONFIG, 128, 4),
             ("sd15_512", V.VAE_SD15_CONFIG, 64, 1)]
    eager = V.build_vae_decoder(V.VAE_SDXL_CONFIG, device=DEV)
    smoke(eager, V.VAE_SDXL_CONFIG, say)
    del eager
    for name, cfg, L, B in cases:
        torch.cuda.empty_cache()
        vae = hip_graph_opt(V.build_vae_decoder(cfg, device=DEV))
        z = _latents(cfg, B, L)
        runs = {"ours": lambda: vae.decode(z)}
        how = "n/a"
        if not args.no_stock:
            stock = vae_ref.stock_decoder(cfg, vae.state_dict(), torch.float16, DEV).to(memory_format=torch.channels_last)
            with torch.no_grad():
                ref = stock(z)
            try:
                hip_graph_opt(stock)
                with torch.no_grad():
                    stock(z)
                how = "hipGraph"
            except Exception as e:            # a stock operator that cannot be captured: timed eager
                stock = vae_ref.stock_decoder(cfg, vae.state_dict(), torch.float16, DEV).to(memory_format=torch.channels_last)
                how = "eager (capture failed: %s)" % type(e).__name__

            def run_stock():
                with torch.no_grad():
                    stock(z)
            runs["stock"] = run_stock
        for fn in runs.values():
            fn(); fn()
        t = {k: [] for k in runs}
        for _ in range(args.repeats):          # alternating
            for k, fn in runs.items():
                t[k].append(_timed(fn))
        rec = dict(case=name, batch=B, latent=L, repeats=args.repeats, stock_run=how)
        for k, v in t.items():
            rec[k + "_ms"] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
        if "stock" in t:
            rec["stock_over_ours"] = round(statistics.median(t["stock"]) / statistics.median(t["ours"]), 3)
            rec["max_abs_diff_vs_stock_fp16"] = float((vae.decode(z).float() - ref.float()).abs().max())
        say(json.dumps(rec))
        del vae, runs
        if not args.no_stock:
            del stock
    if not args.no_kernel_stats:
        kernel_stats(say)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
