"""Decoupled cross-attention (IP-Adapter): the one launch (mixdq_attention_f16_ip) against the chain it replaces --
attention_f16 per key set, torch half operations, quantize_per_tensor_to_int8 -- both replayed from a captured graph
with to_out.0's INT8 operand as the result (the chain scales with a host scalar, `acc + 0.6 * o_j`: the shortest chain a
user could write, not `_C.attention_ip`'s capturable fallback, which has more launches).  SDXL's two cross-attention
shapes, batch 1 and a guided pair of rows.  Then a whole SDXL UNet forward with and without an adapter (unet_steps).
`--model sd15`: the same at SD 1.5's four cross-attention shapes at 512 px (eight heads of 40 / 80 / 160 columns:
mixdq_attention_f16_ip_hd) and on the SD 1.5 UNet.

    python tools/bench_ip_adapter.py [--model sdxl|sd15] [--out profiles/ip_adapter[_hd]_bench.txt] [--rounds 7] [--replays 1000]

Each figure is the median over `rounds` of the time of `replays` graph replays of 10 launches (device events),
the two forms alternating within a round; the spread is min .. max of the rounds.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mixdq_amd._C as C  # noqa: E402

# (query tokens, channels, heads) of the cross-attentions: SDXL's two transformer levels at 1024 px; SD 1.5's at 512 px
SHAPES = {"sdxl": [(4096, 640, 10), (1024, 1280, 20)],
          "sd15": [(4096, 320, 8), (1024, 640, 8), (256, 1280, 8), (64, 1280, 8)]}
PER_GRAPH = 10


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


def unet_steps(dev, args):
    """A whole UNet forward (SDXL at 1024 px or SD 1.5 at 512 px, uniform W8A8 + BOS, fused, from a graph) without an
    adapter, with one 4-token adapter at scale 0.6, and with that adapter at scale 0 -- every cross-attention then runs
    to_q as its own GEMM and a text-only mixdq_attention_f16_ip[_hd] launch where SDXL's plain forward has the one-launch
    to_q + cross-attention at batch 1: that difference is the price of the lost fusion (SD 1.5's plain forward has no
    such launch: nothing is lost there)."""
    import bench
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.ip_adapter import IPState, build_ip_adapter
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import SD15_CONFIG, SDXL_CONFIG, build_unet, quantizable_layers
    cfg, latent, embed = (SDXL_CONFIG, 128, 1280) if args.model == "sdxl" else (SD15_CONFIG, 64, 1024)
    out = [f"# whole {args.model} UNet forward, ms: plain | adapter, scale 0.6 | adapter, scale 0 (text-only launches); median "
           f"[min .. max] of {args.rounds} alternating rounds of 10 replays"]
    unet = build_unet(dev, cfg=cfg)
    adapter = build_ip_adapter(cfg, embed, device=dev)
    for B in (1, 2):
        inp = example_inputs(B, latent, dev, seed=42, cfg=cfg)
        if B == 1:
            with torch.no_grad():
                ckpt = calibrate(unet, [inp])
            names = list(quantizable_layers(unet))
            act = {n: 8 for n in names if args.model == "sdxl" or n not in ("conv_in", "conv_out")}
            quantize_unet(unet, bench.Cfg({n: 8 for n in names}, act), ckpt, bos=True,
                          bos_dict=precompute_bos(unet, inp["encoder_hidden_states"]))
            unet.set_fused(True)
        ip = IPState([adapter.kv(adapter.tokens(torch.randn(B, embed, device=dev).half()))],
                     torch.full((len(adapter.dims), 1), 0.6, device=dev))
        with torch.no_grad():
            graphs = {}
            for name, fn in (("plain", lambda: unet(**inp)[0]), ("ip", lambda: unet(**inp, ip=ip)[0])):
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                graphs[name] = g
        runs = (("plain", graphs["plain"], None), ("ip 0.6", graphs["ip"], 0.6), ("ip 0", graphs["ip"], 0.0))
        ms = {k: [] for k, _, _ in runs}
        for r in range(args.rounds + 1):
            for k, g, sc in runs:
                if sc is not None:
                    ip.scales.fill_(sc)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(10):
                    g.replay()
                b.record()
                torch.cuda.synchronize()
                if r:
                    ms[k].append(a.elapsed_time(b) / 10)
        out.append(f"batch {B}:  " + "   ".join(f"{k} {statistics.median(v):7.3f} [{min(v):7.3f} .. {max(v):7.3f}]"
                                               for k, v in ms.items()))
        print(out[-1], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("sdxl", "sd15"), default="sdxl")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=1000)
    args = ap.parse_args()
    args.out = args.out or os.path.join("profiles", "ip_adapter_bench.txt" if args.model == "sdxl" else "ip_adapter_hd_bench.txt")
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen, dtype=torch.float32).half()
    si, zp = torch.tensor(23.0, device=dev), torch.tensor(3.0, device=dev)
    lines = [f"# {torch.cuda.get_device_name(0)}; us per cross-attention, INT8 output; median of {args.rounds} rounds "
             f"[min .. max], {args.replays} replays x {PER_GRAPH} launches per round",
             "# tq    C  B  image tokens   one launch               chain                    chain / one"]
    for tq, ch, heads in SHAPES[args.model]:
        for B in (1, 2):
            for tokens in ((4,), (16,), (4, 4), (16, 16)):
                q, kv = rnd(B, tq, ch), rnd(B, 77, 2 * ch)
                k, v = kv[..., :ch], kv[..., ch:]
                ip = [(t[..., :ch], t[..., ch:]) for t in (rnd(B, n, 2 * ch) for n in tokens)]
                s = torch.full((len(tokens),), 0.6, device=dev)

                def one():
                    return C.attention_ip(q, k, v, ip, s, heads, si, zp)

                def chain():
                    acc = C.attention_f16(q, k, v, heads)
                    for j, (kj, vj) in enumerate(ip):
                        acc = acc + 0.6 * C.attention_f16(q, kj, vj, heads)
                    return C.quantize_per_tensor_to_int8(acc, si, zp)

                (g1, o1), (g2, o2) = capture(one), capture(chain)
                for g in (g1, g2):                       # warm up; the outputs exist once a graph has run
                    time_us(g, args.replays)
                assert torch.equal(o1, o2), "the two forms disagree"
                t1, t2 = [], []
                for _ in range(args.rounds):
                    t1.append(time_us(g1, args.replays))
                    t2.append(time_us(g2, args.replays))
                m1, m2 = statistics.median(t1), statistics.median(t2)
                lines.append(f"{tq:5d} {ch:4d} {B:2d}  {str(tokens):13s} {m1:7.2f} [{min(t1):6.2f} .. {max(t1):6.2f}]   "
                             f"{m2:7.2f} [{min(t2):6.2f} .. {max(t2):6.2f}]   {m2 / m1:5.2f}")
                print(lines[-1], flush=True)
    lines += unet_steps(dev, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
