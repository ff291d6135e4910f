"""Time the LoHa + DoRA switch on one MI355X: `LoraBank.apply` of one rank-32 LoHa adapter and one rank-64 DoRA adapter
over every Linear and conv of a built, quantized SDXL or SD 1.5 UNet (tools/bench_lora.py's build), `set_scales` alone, the
bare `_C.lycoris_requant` launch inside them, `_C.lora_requant` at the same summed rank (96) on the same layers, the torch
chain that does the same per layer from the same masters, and the HBM floor of the bytes the launch must move.

    python tools/bench_lycoris.py [--model sdxl|sd15] [--rule absmax|keep] [--rounds 5] [--out profiles/lycoris_bench.txt]

Host clock around work that ends in a device synchronise; medians of alternating rounds after one warm-up round."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_lora import HBM_BYTES_PER_S, build, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sdxl", choices=("sdxl", "sd15"))
    ap.add_argument("--rule", default="absmax", choices=("absmax", "keep"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lycoris.py measures on the GPU"
    import mixdq_amd._C as C
    from mixdq_amd.lora import LoraBank
    dev, RH, RD = "cuda:0", 32, 64
    unet, state, inp = build(a.model, dev)
    bank = LoraBank(unet, state, bos_embedding=inp["encoder_hidden_states"][0, 0], max_rank=RH + RD, scales=a.rule)
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda s, *shape: (torch.randn(shape, generator=g, device=dev) * s).half()      # noqa: E731
    loha, dora, plain = {}, {}, {}
    for name, mod in bank.modules.items():
        w = state[name + ".weight"]
        n, rest = w.shape[0], tuple(w.shape[1:])
        loha[name] = dict(kind="loha", w1_a=rnd(0.2, n, RH), w1_b=rnd(0.2, RH, *rest), w2_a=rnd(0.2, n, RH), w2_b=rnd(0.2, RH, *rest),
                          alpha=float(RH))
        dora[name] = dict(kind="lora", A=rnd(0.1, RD, *rest), B=rnd(0.05, n, RD), alpha=float(RD))
        if not getattr(mod, "split", 0) or not mod.valid_for_acceleration:      # (a split shortcut takes no magnitude)
            dora[name]["magnitude"] = w.float().flatten(1).norm(dim=1).to(dev)
        plain[name] = (rnd(0.1, RH + RD, *rest), rnd(0.05, n, RH + RD), float(RH + RD))
    apply = lambda: bank.apply([loha, dora], [0.75, 0.75])     # noqa: E731
    scales = lambda: bank.set_scales([0.5, 0.5])               # noqa: E731
    apply()
    targets = [t for ts in bank.targets.values() for t in ts]
    table = bank.lyco["table"]
    launch = lambda: C.lycoris_requant(table)                  # noqa: E731
    lora_launch = lambda: C.lora_requant(bank.table)           # noqa: E731  (reads Bcat | Acat over all 96 ranks as linear)

    def chain():                                               # what a user would write per layer, from the same masters
        for t in targets:
            bs = t.Bcat.float() * t.svec
            wp = (t.keep[0][:, t.col0:t.col0 + t.kf].float() + bs[:, :RD] @ t.Acat[:RD].float()
                  + (bs[:, RD:] @ t.Acat[RD:].float()) * (t.B2cat[:, RD:].float() @ t.A2cat[RD:].float()))
            if t.mag is not None:
                wp = wp * (t.mag / wp.norm(dim=1))[:, None]
            if t.desc.mode == C.LORA_F16:
                t.Bcat.new_empty(wp.shape).copy_(wp)
                continue
            d = wp.abs().amax(1) / 127 if a.rule == "absmax" else getattr(t.mod, "weight_scales" + t.sfx)
            q = torch.quantize_per_channel(wp, d, torch.zeros_like(d), 0, torch.qint8).int_repr()
            s = q.view(q.shape[0], t.kf // t.desc.tap_len, -1).float().sum(2)
            s * getattr(t.mod, "act_zero_points" + t.sfx), d * getattr(t.mod, "act_scales" + t.sfx)

    forms = (("apply", apply), ("set_scales", scales), ("launch", launch), ("lora", lora_launch), ("chain", chain))
    ms = {k: [] for k, _ in forms}
    for r in range(a.rounds + 1):                              # alternating; round 0 is the warm-up
        for k, fn in forms:
            v = timed(fn)
            if r:
                ms[k].append(v)
    bank.restore()
    # two reads of the master (the norm or ABSMAX forces the first pass on every layer here), one write, the factors once
    moved = sum(t.N * t.kf * (2 * 2 + (2 if t.desc.mode == C.LORA_F16 else 1)) + 2 * (RD + 2 * RH) * (t.N + t.kf) for t in targets)
    lines = [f"{a.model} {a.rule}: {len(targets)} descriptors, {sum(t.N * t.kf for t in targets) / 1e9:.2f} G weights, "
             f"LoHa rank {RH} + DoRA rank {RD}, grid {table.grid}"]
    for k, label in (("apply", "bank.apply"), ("set_scales", "bank.set_scales"), ("launch", "  its lycoris_requant launch"),
                     ("lora", "lora_requant launch, rank 96"), ("chain", "torch chain, per layer")):
        lines.append(f"  {label:30s} median {statistics.median(ms[k]):9.3f} ms  (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})")
    floor = moved / HBM_BYTES_PER_S * 1e3
    lines.append(f"  HBM floor of the launch        {floor:9.3f} ms  ({moved / 1e9:.2f} GB at 8 TB/s): the launch is "
                 f"{statistics.median(ms['launch']) / floor:.1f}x above it")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
