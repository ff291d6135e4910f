"""Time the LoRA switch on one MI355X: `LoraBank.apply` of one rank-64 adapter over every Linear and conv of a built,
quantized SDXL or SD 1.5 UNet (uniform W8A8 + BOS, fused, synthetic weights), `set_scales` alone, the bare
`_C.lora_requant` launch inside them, the torch chain that does the same per layer from the same masters (FP32 product,
add, per-channel quantize or FP16 cast, sums), and the HBM floor of the bytes the launch must move.

    python tools/bench_lora.py [--model sdxl|sd15] [--rule absmax|keep] [--rounds 5] [--out profiles/lora_bench.txt]

Host clock around work that ends in a device synchronise (apply and set_scales have host work: factor copies, the BOS
rows, the refresh_derived_() walk); medians of alternating rounds after one warm-up round.  The peak of
torch.cuda.max_memory_allocated over the allocation level before the call is reported for the first apply() (which
builds masters, factor buffers and tables), for a later one, and for set_scales."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_BYTES_PER_S = 8.0e12        # MI355X peak


def build(model, dev):
    import bench
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import SD15_CONFIG, SDXL_CONFIG, build_unet, quantizable_layers
    cfg, latent = (SDXL_CONFIG, 128) if model == "sdxl" else (SD15_CONFIG, 64)
    unet = build_unet(dev, cfg=cfg)
    state = {k: v.detach().clone() for k, v in unet.state_dict().items() if k.endswith(".weight")}
    inp = example_inputs(1, latent, dev, seed=42, cfg=cfg)
    with torch.no_grad():
        ckpt = calibrate(unet, [inp])
    names = list(quantizable_layers(unet))
    act = {n: 8 for n in names if model == "sdxl" or n not in ("conv_in", "conv_out")}
    quantize_unet(unet, bench.Cfg({n: 8 for n in names}, act), ckpt, bos=True,
                  bos_dict=precompute_bos(unet, inp["encoder_hidden_states"]))
    unet.set_fused(True)
    return unet, state, inp


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def peak_over(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sdxl", choices=("sdxl", "sd15"))
    ap.add_argument("--rule", default="absmax", choices=("absmax", "keep"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lora.py measures on the GPU"
    import mixdq_amd._C as C
    from mixdq_amd.lora import LoraBank
    dev, R = "cuda:0", a.rank
    unet, state, inp = build(a.model, dev)
    bank = LoraBank(unet, state, bos_embedding=inp["encoder_hidden_states"][0, 0], max_rank=R, scales=a.rule)
    g = torch.Generator(device=dev).manual_seed(0)
    adapter = {}
    for name in bank.modules:
        w = state[name + ".weight"]
        adapter[name] = ((torch.randn((R,) + tuple(w.shape[1:]), generator=g, device=dev) * 0.1).half(),
                         (torch.randn((w.shape[0], R), generator=g, device=dev) * 0.05).half(), float(R))
    apply = lambda: bank.apply([adapter], [0.75])              # noqa: E731
    scales = lambda: bank.set_scales([0.5])                    # noqa: E731
    launch = lambda: C.lora_requant(bank.table)                # noqa: E731
    first_mb = peak_over(apply)
    targets = [t for ts in bank.targets.values() for t in ts]

    def chain():                                               # what a user would write per layer, from the same masters
        for t in targets:
            wp = t.keep[0][:, t.col0:t.col0 + t.kf].float() + (t.Bcat.float() * t.svec) @ t.Acat.float()
            if t.desc.mode == C.LORA_F16:
                t.Bcat.new_empty(wp.shape).copy_(wp)
                continue
            d = wp.abs().amax(1) / 127 if a.rule == "absmax" else getattr(t.mod, "weight_scales" + t.sfx)
            q = torch.quantize_per_channel(wp, d, torch.zeros_like(d), 0, torch.qint8).int_repr()
            s = q.view(q.shape[0], t.kf // t.desc.tap_len, -1).float().sum(2)
            s * getattr(t.mod, "act_zero_points" + t.sfx), d * getattr(t.mod, "act_scales" + t.sfx)

    forms = (("apply", apply), ("set_scales", scales), ("launch", launch), ("chain", chain))
    ms = {k: [] for k, _ in forms}
    for r in range(a.rounds + 1):                              # alternating; round 0 is the warm-up
        for k, fn in forms:
            v = timed(fn)
            if r:
                ms[k].append(v)
    later_mb, scales_mb = peak_over(apply), peak_over(scales)
    bank.restore()
    moved = sum(t.N * t.kf * (2 * (2 if a.rule == "absmax" and t.desc.mode != C.LORA_F16 else 1) + (2 if t.desc.mode == C.LORA_F16 else 1))
                + 2 * R * (t.N + t.kf) for t in targets)
    weights = sum(t.N * t.kf for t in targets)
    lines = [f"{a.model} {a.rule}: {len(targets)} descriptors, {weights / 1e9:.2f} G weights, rank {R}, grid {bank.table.grid}"]
    for k, label in (("apply", "bank.apply"), ("set_scales", "bank.set_scales"), ("launch", "  its lora_requant launch"),
                     ("chain", "torch chain, per layer")):
        lines.append(f"  {label:26s} median {statistics.median(ms[k]):9.3f} ms  (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})")
    lines += [f"  HBM floor of the launch    {moved / HBM_BYTES_PER_S * 1e3:9.3f} ms  ({moved / 1e9:.2f} GB at 8 TB/s)",
              f"  peak device memory over the level before the call: first apply {first_mb:.1f} MiB (masters, factor buffers, "
              f"tables, BOS base rows), a later apply {later_mb:.1f} MiB, set_scales {scales_mb:.1f} MiB"]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
