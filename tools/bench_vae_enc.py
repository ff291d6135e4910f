"""Latency of the FP16 VAE encoder (mixdq_amd.vae.VAEEncoder) next to the same network on stock PyTorch, same box.

    python tools/bench_vae_enc.py [--repeats 7] [--out profiles/vae_enc_bench.txt] [--step-timeout 420]

Synthetic weights (build_vae_encoder, seed 42) -- every number below is with them.  The run is a chain of steps, each a
child process of its own under its own time limit; the chain stops at the first step that fails or runs out of time:
  smoke       one eager 1024-px encode: finite, and the launch audit (torch.profiler) -- which kernels are this
              library's, which are not (the copy of the noise into channels-last storage is the only one expected)
  conv_in     conv_in at 1024 px, batch 1, on both routes, once: the ingest to 8 channels + the zero-padded weight on
              the MFMA tiles, against the 3-channel FP16 image on the one-output-per-thread kernel
  sdxl_1024_b1, sdxl_1024_b4, sd15_512_b1
              ours    hipGraph replays of VAEEncoder.encode(image, noise) from a uint8 image (hip_graph_opt)
              stock   the encoder of tests/vae_enc_ref.py (nn.Conv2d / nn.GroupNorm / F.pad / SDPA) in FP16,
                      channels-last, from the FP16 image, under the same capture where the stock operators can be
                      captured, else eager (the line says which); it stops at the moments (no posterior sample)
              alternating, `--repeats` timed runs each after 2 untimed ones; a run is timed on the host clock from the
              call to a device synchronise behind it.  Reported: median and [min, max].
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
STEPS = ("smoke", "conv_in", "sdxl_1024_b1", "sdxl_1024_b4", "sd15_512_b1")


def _timed(fn):
    import torch
    torch.cuda.synchronize(DEV)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(DEV)
    return 1e3 * (time.perf_counter() - t0)


def _inputs(B, px, seed=5):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    pixels = torch.randint(0, 256, (B, 3, px, px), generator=g, dtype=torch.uint8).to(DEV)
    noise = torch.randn(B, 4, px // 8, px // 8, generator=g).to(DEV)
    return pixels, noise


def step_smoke(say, args):
    import torch
    from torch.profiler import ProfilerActivity, profile
    from mixdq_amd import vae as V
    say("# tools/bench_vae_enc.py -- synthetic weights; %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    enc = V.build_vae_encoder(V.VAE_SDXL_CONFIG, device=DEV)
    pixels, noise = _inputs(1, 1024)
    z = enc.encode(pixels, noise)
    torch.cuda.synchronize(DEV)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        enc.encode(pixels, noise)
        torch.cuda.synchronize(DEV)
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
             and "Memcpy" not in e.name and "Memset" not in e.name]
    ours, other = [n for n in names if "mixdq" in n], [n for n in names if "mixdq" not in n]
    forms = {k: sum(k in n for n in ours) for k in ("image_to_nhwc8", "vae_latent", "igemm_kernel", "f16_generic",
                                                    "attn_512", "gn_")}
    finite = bool(torch.isfinite(z).all())
    say(json.dumps(dict(smoke="1024 px encode", shape=list(z.shape), finite=finite, abs_max=float(z.abs().max()),
                        library_kernels=len(ours), by_name=forms, other_kernels=other)))
    if not finite:
        raise SystemExit("bench_vae_enc: the 1024-px encode is not finite")
    if len(other) > 1 or not all("copy" in n.lower() or "elementwise" in n.lower() for n in other):
        raise SystemExit("bench_vae_enc: an encode launches kernels that are not this library's: %r" % other)


def step_conv_in(say, args):
    import torch
    from mixdq_amd import _C
    from mixdq_amd import vae as V
    enc = V.build_vae_encoder(V.VAE_SDXL_CONFIG, device=DEV)
    pixels, _ = _inputs(1, 1024)
    w8, b = enc._derived()["conv_in"]
    w3 = enc.encoder.conv_in.weight
    x3 = V.from_uint8(pixels).contiguous(memory_format=torch.channels_last)
    n = 10
    routes = {"ingest_only": lambda: _C.image_to_nhwc8_f16(pixels),
              "ingest_plus_mfma_conv_8ch": lambda: _C.conv2d_f16(_C.image_to_nhwc8_f16(pixels), w8, b, 1, 1),
              "one_output_per_thread_conv_3ch": lambda: _C.conv2d_f16(x3, w3, b, 1, 1)}
    same = torch.equal(routes["ingest_plus_mfma_conv_8ch"]().float(), routes["one_output_per_thread_conv_3ch"]().float())
    rec = dict(conv_in="1024 px, batch 1, eager, %d back-to-back calls per timing" % n, bit_equal_routes=same)
    for k, fn in routes.items():
        fn(); fn()
        ts = [_timed(lambda: [fn() for _ in range(n)]) / n for _ in range(args.repeats)]
        rec[k + "_ms"] = dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))
    say(json.dumps(rec))


def step_case(say, args, name, cfg_name, px, B):
    import torch
    from mixdq_amd import vae as V
    from mixdq_amd.quantize_sdxl import hip_graph_opt
    from tests import vae_enc_ref
    cfg = getattr(V, cfg_name)
    enc = hip_graph_opt(V.build_vae_encoder(cfg, device=DEV))
    pixels, noise = _inputs(B, px)
    image = V.from_uint8(pixels).contiguous(memory_format=torch.channels_last)
    runs = {"ours": lambda: enc.encode(pixels, noise)}
    stock = vae_enc_ref.stock_encoder(cfg, enc.state_dict(), torch.float16, DEV).to(memory_format=torch.channels_last)
    ref = stock(image)
    try:
        hip_graph_opt(stock)
        stock(image)
        how = "hipGraph"
    except Exception as e:            # a stock operator that cannot be captured: timed eager
        stock = vae_enc_ref.stock_encoder(cfg, enc.state_dict(), torch.float16, DEV).to(memory_format=torch.channels_last)
        how = "eager (capture failed: %s)" % type(e).__name__
    runs["stock"] = lambda: stock(image)
    for fn in runs.values():
        fn(); fn()
    t = {k: [] for k in runs}
    for _ in range(args.repeats):          # alternating
        for k, fn in runs.items():
            t[k].append(_timed(fn))
    rec = dict(case=name, batch=B, px=px, repeats=args.repeats, stock_run=how)
    for k, v in t.items():
        rec[k + "_ms"] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
    rec["stock_over_ours"] = round(statistics.median(t["stock"]) / statistics.median(t["ours"]), 3)
    rec["max_abs_moments_diff_vs_stock_fp16"] = float((enc.moments(pixels).float() - ref.float()).abs().max())
    say(json.dumps(rec))


CASES = {"sdxl_1024_b1": ("VAE_SDXL_CONFIG", 1024, 1), "sdxl_1024_b4": ("VAE_SDXL_CONFIG", 1024, 4),
         "sd15_512_b1": ("VAE_SD15_CONFIG", 512, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds each step may take")
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--step", default=None, help="(child) run this one step in this process")
    args = ap.parse_args()
    if args.step:
        say = lambda s: print(s, flush=True)
        if args.step == "smoke":
            return step_smoke(say, args)
        if args.step == "conv_in":
            return step_conv_in(say, args)
        return step_case(say, args, args.step, *CASES[args.step])
    # the driver: never touches the GPU itself; one child per step, each under its own limit, chained
    lines, status = [], 0
    for step in args.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--repeats", str(args.repeats)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                               timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            lines.append("step %s: no result within %d s; the chain stops here" % (step, args.step_timeout))
            status = 124
            break
        lines += r.stdout.splitlines()
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            lines.append("step %s: exit %d; the chain stops here\n%s" % (step, r.returncode, r.stderr[-1500:]))
            status = r.returncode
            break
    if status:
        print(lines[-1], flush=True)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
