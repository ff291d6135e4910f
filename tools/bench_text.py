"""Latency of the FP16 text encoders (mixdq_amd.text) next to the same networks on stock PyTorch, same box, same process.

    python tools/bench_text.py [--repeats 7] [--out profiles/text_bench.txt] [--no-kernel-stats]

Synthetic weights (build_text_encoder, seed 42) and random token ids (there is no tokenizer here) -- every number
below is with them.  Cases: SDXL's two encoders (CLIP ViT-L/14 + OpenCLIP bigG/14, encode_sdxl) and CLIP-L alone
(encode_sd15), 77 tokens, at batch 1 and 4.  Per case:
  ours    hipGraph replays of this path (hip_graph_opt)
  stock   the encoders of tests/text_ref.py (nn.Embedding / nn.LayerNorm / nn.Linear /
          F.scaled_dot_product_attention(is_causal=True)) in FP16, under the same capture where the stock operators can
          be captured, else eager (the line says which)
alternating, `--repeats` timed runs each after 2 untimed ones; a run is timed on the host clock from the call to a
device synchronise behind it.  Reported: median and [min, max], the number of device kernels of one eager forward and
how many of them are this library's (torch.profiler).
Last, unless --no-kernel-stats: one child process under `rocprofv3 --kernel-trace --stats` runs twenty eager batch-1
SDXL encodes; the per-kernel table is appended.
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
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
T_TOKENS = 77


def _timed(fn):
    torch.cuda.synchronize(DEV)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(DEV)
    return 1e3 * (time.perf_counter() - t0)


def _ids(B, vocab, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ids = torch.randint(0, vocab - 1, (B, T_TOKENS), generator=g)
    ids[:, 9] = vocab - 1                    # the EOS position
    return ids.to(DEV)


class Ours(nn.Module):
    """The case's encoders behind one forward (so that one graph holds the whole case)."""

    def __init__(self, encs):
        super().__init__()
        self.encs = nn.ModuleList(encs)

    @torch.no_grad()
    def forward(self, *ids):
        from mixdq_amd import text as T
        if len(self.encs) == 2:
            return T.encode_sdxl(self.encs[0], self.encs[1], *ids)
        return T.encode_sd15(self.encs[0], ids[0])


class Stock(nn.Module):
    def __init__(self, encs):
        super().__init__()
        self.encs = nn.ModuleList(encs)

    @torch.no_grad()
    def forward(self, *ids):
        if len(self.encs) == 2:
            (_, pen_l, _), (_, pen_g, pooled) = self.encs[0](ids[0]), self.encs[1](ids[1])
            return torch.cat([pen_l, pen_g], dim=-1), pooled
        return self.encs[0](ids[0])[0]


def kernel_audit(fn):
    """Names of the device kernels of one eager run, split into this library's and the rest."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize(DEV)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize(DEV)
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
             and "Memcpy" not in e.name and "Memset" not in e.name]
    return [n for n in names if "mixdq" in n], [n for n in names if "mixdq" not in n]


def encode_loop(n):
    from mixdq_amd import text as T
    m = Ours([T.build_text_encoder(T.CLIP_L_CONFIG, device=DEV), T.build_text_encoder(T.OPENCLIP_BIGG_CONFIG, device=DEV)])
    ids = (_ids(1, 49408, 5), _ids(1, 49408, 6))
    for _ in range(n):
        m(*ids)
    torch.cuda.synchronize(DEV)


def kernel_stats(say):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--encode-loop", "20"]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            say("kernel stats: rocprofv3 run failed (exit %d)\n%s" % (r.returncode, r.stdout[-1500:]))
            return
        say("per-kernel statistics of twenty eager SDXL encodes (both encoders), batch 1 (rocprofv3 --kernel-trace --stats), "
            "by total time:")
        say("  %-8s %10s %10s %7s  %s" % ("calls", "total ms", "avg us", "%", "kernel"))
        import csv
        with open(files[0], newline="") as f:
            for i, row in enumerate(csv.DictReader(f)):
                if i < 16:
                    say("  %-8s %10.3f %10.1f %7.2f  %s" % (row["Calls"], float(row["TotalDurationNs"]) / 1e6,
                                                          float(row["AverageNs"]) / 1e3, float(row["Percentage"]),
                                                          row["Name"][:150]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-kernel-stats", action="store_true")
    ap.add_argument("--no-stock", action="store_true")
    ap.add_argument("--encode-loop", type=int, default=0, help="(child of the rocprofv3 run) eager batch-1 SDXL encodes")
    args = ap.parse_args()
    if args.encode_loop:
        return encode_loop(args.encode_loop)
    from mixdq_amd import text as T
    from mixdq_amd.quantize_sdxl import hip_graph_opt
    from tests import text_ref
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# tools/bench_text.py -- synthetic weights, random token ids; %s; torch %s"
        % (torch.cuda.get_device_name(0), torch.__version__))
    cases = [("sdxl_clip_l+bigg", (T.CLIP_L_CONFIG, T.OPENCLIP_BIGG_CONFIG)), ("sd15_clip_l", (T.CLIP_L_CONFIG,))]
    for name, cfgs in cases:
        torch.cuda.empty_cache()
        encs = [T.build_text_encoder(c, seed=42 + i, device=DEV) for i, c in enumerate(cfgs)]
        eager = Ours(encs)
        stock_encs = None if args.no_stock else [text_ref.stock_encoder(c, e.state_dict(), torch.float16, DEV)
                                                 for c, e in zip(cfgs, encs)]
        for B in (1, 4):
            ids = tuple(_ids(B, c["vocab_size"], 5 + i) for i, c in enumerate(cfgs))
            ours_k, other_k = kernel_audit(lambda: eager(*ids))
            out = eager(*ids)
            first = out[0] if isinstance(out, tuple) else out
            if not bool(torch.isfinite(first).all()):
                raise SystemExit("bench_text: the encoding is not finite")
            ours = hip_graph_opt(Ours(encs))
            runs = {"ours": lambda: ours(*ids)}
            how = "n/a"
            rec = dict(case=name, batch=B, tokens=T_TOKENS, repeats=args.repeats, launches=len(ours_k) + len(other_k),
                       library_launches=len(ours_k), other_kernels=sorted(set(n[:60] for n in other_k)))
            if stock_encs is not None:
                stock = Stock(stock_encs)
                ref = stock(*ids)
                s_k, s_other = kernel_audit(lambda: stock(*ids))
                rec["stock_launches"] = len(s_k) + len(s_other)
                try:
                    stock = hip_graph_opt(Stock(stock_encs))
                    stock(*ids)
                    how = "hipGraph"
                except Exception as e:            # a stock operator that cannot be captured: timed eager
                    stock = Stock(stock_encs)
                    how = "eager (capture failed: %s)" % type(e).__name__
                runs["stock"] = lambda: stock(*ids)
            rec["stock_run"] = how
            for fn in runs.values():
                fn(); fn()
            t = {k: [] for k in runs}
            for _ in range(args.repeats):          # alternating
                for k, fn in runs.items():
                    t[k].append(_timed(fn))
            for k, v in t.items():
                rec[k + "_ms"] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
            if "stock" in t:
                rec["stock_over_ours"] = round(statistics.median(t["stock"]) / statistics.median(t["ours"]), 3)
                ref0 = ref[0] if isinstance(ref, tuple) else ref
                rec["max_abs_diff_vs_stock_fp16"] = float((first.float() - ref0.float()).abs().max())
            say(json.dumps(rec))
            del ours, runs
        del encs, eager, stock_encs
    if not args.no_kernel_stats:
        kernel_stats(say)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
