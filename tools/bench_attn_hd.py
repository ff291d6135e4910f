"""Microbenchmark of the FP16 attention core at SD 1.5's head widths (hipGraph-timed, tools/bench_attn.py's timer).

    python tools/bench_attn_hd.py [--bs 1,2] [--repeats 3] [--out profiles/attn_hd_bench.txt]

Per shape of the SD 1.5 UNet at 512 px (8 heads: D = C / 8) and batch: us per launch of the HIP kernel, of PyTorch's
FP16 SDPA on the same tensors, and of the head_dim-64 kernel on the same token counts and C (C / 64 heads: the same
FLOPs), the per-FLOP yardstick.  On the cross-attention rows (77 keys) two more columns: the short-key form (`_cfg=1`)
and the tiled kernel in the form it would take without one (`_cfg=4` / `2` by the library's own rule); `hip us` is the
automatic routing.  `--repeats N` measures the whole table N times: the run-to-run spread of this tool on this box."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_attn import timed  # noqa: E402

SHAPES = [  # (name, Tq, Tkv, C)
    ("self 64x64 C320", 4096, 4096, 320), ("self 32x32 C640", 1024, 1024, 640), ("self 16x16 C1280", 256, 256, 1280),
    ("cross 64x64 C320", 4096, 77, 320), ("cross 32x32 C640", 1024, 77, 640), ("cross 16x16 C1280", 256, 77, 1280),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", default="1,2")
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=1)
    a = ap.parse_args()
    from mixdq_amd import _C
    dev = torch.device("cuda:0")
    rows = []
    for rep_i, bs in ((r, int(x)) for r in range(a.repeats) for x in a.bs.split(",")):
        for name, tq, tkv, c in SHAPES:
            torch.manual_seed(0)
            if tq == tkv:
                qkv = torch.randn(bs, tq, 3 * c, device=dev, dtype=torch.float16)
                q, k, v = qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:]
            else:
                q = torch.randn(bs, tq, c, device=dev, dtype=torch.float16)
                kv = torch.randn(bs, tkv, 2 * c, device=dev, dtype=torch.float16)
                k, v = kv[..., :c], kv[..., c:]
            h, d = 8, c // 8

            def sdpa():
                return F.scaled_dot_product_attention(*(x.unflatten(-1, (h, d)).transpose(1, 2) for x in (q, k, v))
                                                      ).transpose(1, 2).reshape(bs, tq, c)
            row = {"shape": name, "bs": bs, "rep": rep_i, "head_dim": d, "gflop": round(4 * bs * tq * tkv * c / 1e9, 3),
                   "hip_us": round(timed(lambda: _C.attention_f16(q, k, v, h)), 2),
                   "sdpa_us": round(timed(sdpa), 2),
                   "hip_d64_us": round(timed(lambda: _C.attention_f16(q, k, v, c // 64)), 2)}
            if tkv <= 128:      # the two forms side by side (the tiled one as the library sizes it: csrc/attention.hip)
                tiled = 4 if ((tq + 127) // 128) * h >= 128 else 2
                row["form1_us"] = round(timed(lambda: _C.attention_f16(q, k, v, h, _cfg=1)), 2)
                row["tiled_us"] = round(timed(lambda: _C.attention_f16(q, k, v, h, _cfg=tiled)), 2)
                row["tiled_form"] = tiled
            row["hip_tflops"] = round(row["gflop"] / row["hip_us"] * 1e3, 1)
            row["hip_over_sdpa"] = round(row["hip_us"] / row["sdpa_us"], 2)
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_attn_hd.py: us per launch, hipGraph-timed; hip_d64 = the head_dim-64 kernel on "
                    "the same tensors (C / 64 heads, same FLOPs)\n")
            f.write("# form1 = the short-key form (_cfg=1), tiled = the tiled kernel forced to the form named behind it; "
                    "rep = repeat of the whole table\n")
            f.write(f"{'shape':<20}{'bs':>3}{'rep':>4}{'D':>5}{'GFLOP':>8}{'hip us':>9}{'sdpa us':>9}{'d64 us':>9}"
                    f"{'hip/sdpa':>9}{'TFLOP/s':>9}{'form1 us':>10}{'tiled us':>10}{'form':>5}\n")
            for r in rows:
                f1 = f"{r['form1_us']:>10.2f}{r['tiled_us']:>10.2f}{r['tiled_form']:>5}" if "form1_us" in r else \
                    f"{'-':>10}{'-':>10}{'-':>5}"
                f.write(f"{r['shape']:<20}{r['bs']:>3}{r['rep']:>4}{r['head_dim']:>5}{r['gflop']:>8.2f}{r['hip_us']:>9.2f}"
                        f"{r['sdpa_us']:>9.2f}{r['hip_d64_us']:>9.2f}{r['hip_over_sdpa']:>9.2f}{r['hip_tflops']:>9.1f}"
                        f"{f1}\n")


if __name__ == "__main__":
    main()
