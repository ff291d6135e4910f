"""The Resampler's launches against what they replace, all replayed from captured graphs, synthetic weights:

  * mixdq_linear_f16_skinny against mixdq_linear_f16 (the LayerNorm forms against the LayerNorm launch + mixdq_linear_f16)
    at the five latent-side shapes of RESAMPLER_PLUS_SD15 / _SDXL, B = 1 and 4, with each shape's weight-streaming floor;
  * mixdq_attention_f16_perceiver against torch.cat + mixdq_attention_f16 at 257 + 16 keys, 12 and 20 heads;
  * a whole Resampler call against the same network from stock torch functions (tests/resampler_ref.py) in FP16.

    python tools/bench_resampler.py [--out profiles/resampler_bench.txt] [--rounds 7] [--replays 200]

Each figure is the median over `rounds` of the time of `replays` graph replays of 10 calls (device events), the two
forms alternating within a round; the spread is min .. max of the rounds.  Replays of one graph re-read the same
weights: they are served from the last-level cache where they fit, so these are warm-cache figures.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mixdq_amd._C as C  # noqa: E402
from mixdq_amd.ip_adapter import RESAMPLER_PLUS_SD15, RESAMPLER_PLUS_SDXL, Resampler  # noqa: E402
from tests import resampler_ref  # noqa: E402

PER_GRAPH = 10
HBM_BYTES_PER_US = 8.0e6                       # MI355X: 8 TB/s


def capture(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(PER_GRAPH):
            out = fn()
    return g, out


def time_us(g, replays):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (replays * PER_GRAPH)


def ab(new, old, args):
    (g1, _), (g2, _) = capture(new), capture(old)
    for g in (g1, g2):
        time_us(g, args.replays)
    t1, t2 = [], []
    for _ in range(args.rounds):
        t1.append(time_us(g1, args.replays))
        t2.append(time_us(g2, args.replays))
    m1, m2 = statistics.median(t1), statistics.median(t2)
    return f"{m1:8.2f} [{min(t1):7.2f} .. {max(t1):7.2f}]   {m2:8.2f} [{min(t2):7.2f} .. {max(t2):7.2f}]   {m2 / m1:5.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "resampler_bench.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen, dtype=torch.float32).half()  # noqa: E731
    lines = [f"# {torch.cuda.get_device_name(0)}; us per call; median of {args.rounds} rounds [min .. max], "
             f"{args.replays} replays x {PER_GRAPH} calls per round; graphs replayed back to back (warm caches)",
             "# few-row GEMM: M  N  K  form | floor (weight bytes / 8 TB/s) | skinny | linear_f16 (LN forms: LayerNorm launch + linear_f16) | old / new"]
    for name, cfg in (("sd15", RESAMPLER_PLUS_SD15), ("sdxl", RESAMPLER_PLUS_SDXL)):
        dim, inner, hid = cfg["dim"], cfg["dim_head"] * cfg["heads"], cfg["dim"] * cfg["ff_mult"]
        out_dim = 768 if name == "sd15" else 2048
        shapes = [("ln qkv", 3 * inner, dim, "ln"), ("to_out+res", dim, inner, "res"), ("ln fc1 gelu", hid, dim, "lngelu"),
                  ("fc2+res", dim, hid, "res"), ("proj_out+bias", out_dim, dim, "bias")]
        for B in (1, 4):
            M = 16 * B
            for label, N, K, form in shapes:
                a, w, bias, res = rnd(M, K), rnd(N, K) * K ** -0.5, rnd(N), rnd(M, N)
                gm, bt = rnd(K), rnd(K)
                if form == "ln":
                    new = lambda: C.linear_f16_skinny(a, w, ln=(gm, bt, 1e-5))  # noqa: E731
                    old = lambda: C.linear_f16(C.layernorm_quantize(a, gm, bt, 1e-5, [], want_f16=True)[1], w)  # noqa: E731
                elif form == "lngelu":
                    new = lambda: C.linear_f16_skinny(a, w, ln=(gm, bt, 1e-5), act="gelu")  # noqa: E731
                    old = lambda: C.linear_f16(C.layernorm_quantize(a, gm, bt, 1e-5, [], want_f16=True)[1], w, _act="gelu")  # noqa: E731
                elif form == "res":
                    new = lambda: C.linear_f16_skinny(a, w, residual=res)  # noqa: E731
                    old = lambda: C.linear_f16(a, w, _residual=res)  # noqa: E731
                else:
                    new = lambda: C.linear_f16_skinny(a, w, bias)  # noqa: E731
                    old = lambda: C.linear_f16(a, w, bias)  # noqa: E731
                lines.append(f"{name} {M:3d} {N:5d} {K:5d}  {label:14s} floor {2 * N * K / HBM_BYTES_PER_US:5.2f}   {ab(new, old, args)}")
                print(lines[-1], flush=True)
    lines.append("# perceiver attention, 16 queries, 257 + 16 keys: B heads | one launch | torch.cat x 2 + attention_f16 | old / new")
    for heads in (12, 20):
        for B in (1, 4):
            Cw = heads * 64
            qkv, img = rnd(B, 16, 3 * Cw), rnd(B, 257, 2 * Cw)
            q, k2, v2, k1, v1 = qkv[..., :Cw], qkv[..., Cw:2 * Cw], qkv[..., 2 * Cw:], img[..., :Cw], img[..., Cw:]
            new = lambda: C.attention_perceiver(q, k1, v1, k2, v2, heads)  # noqa: E731
            old = lambda: C.attention_f16(q, torch.cat([k1, k2], dim=1), torch.cat([v1, v2], dim=1), heads)  # noqa: E731
            lines.append(f"{B:2d} {heads:3d}   {ab(new, old, args)}")
            print(lines[-1], flush=True)
    lines.append("# whole Resampler, 257 hidden states -> 16 tokens: config B | ours | stock torch functions, FP16 | stock / ours")
    for name, cfg, out_dim in (("sd15", RESAMPLER_PLUS_SD15, 768), ("sdxl", RESAMPLER_PLUS_SDXL, 2048)):
        rs = Resampler(num_queries=16, output_dim=out_dim, **cfg).half().to(dev).eval()
        sd = rs.state_dict()
        for B in (1, 4):
            hidden = rnd(B, 257, cfg["embedding_dim"])
            with torch.no_grad():
                new = lambda: rs(hidden)  # noqa: E731
                old = lambda: resampler_ref.forward(sd, hidden, cfg["heads"], cfg["depth"])  # noqa: E731
                lines.append(f"{name} {B:2d}   {ab(new, old, args)}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
