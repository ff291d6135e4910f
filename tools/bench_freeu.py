"""Time FreeU on one MI355X: the `_C.freeu` launch against the torch chain it replaces (diffusers' fourier_filter with
torch.fft in FP32 plus the slice multiply, from and to FP16 channels-last) on the six (hidden, skip) pairs of SDXL at
1024 px and of SD 1.5 at 512 px, batch 1 and a guided pair; and a whole fused W8A8 forward with FreeU off, on, and on at
all-ones.

    python tools/bench_freeu.py [--rounds 7] [--reps 20] [--forward sdxl|sd15|none] [--out profiles/freeu_bench.txt]

Everything is timed from captured graphs (`reps` calls per graph, device events around one replay), the forms alternating
within a round after one warm-up round; medians with the rounds' min and max.  A chain that cannot be captured is timed
eagerly and marked so."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_BYTES_PER_S = 8.0e12        # MI355X peak
PAIRS = {"sdxl": [(1280, 1280, 32), (1280, 1280, 32), (1280, 640, 32), (1280, 640, 64), (640, 640, 64), (640, 320, 64)],
         "sd15": [(1280, 1280, 8), (1280, 1280, 8), (1280, 1280, 8), (1280, 1280, 16), (1280, 1280, 16), (1280, 640, 16)]}


def chain(hidden, skip, b, s):
    """What a patched UpBlock.forward runs today (diffusers' apply_freeu at threshold 1)."""
    half = hidden.shape[1] // 2
    hidden = torch.cat([hidden[:, :half] * b, hidden[:, half:]], dim=1)
    x = skip.float()
    H, W = x.shape[-2:]
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones_like(x)
    mask[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = s
    y = torch.fft.ifftn(torch.fft.ifftshift(f * mask, dim=(-2, -1)), dim=(-2, -1)).real
    return hidden, y.to(skip.dtype)


def graphed(fn, reps):
    """replay() of a graph holding `reps` calls of fn, or None where the capture fails."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
    except RuntimeError:
        torch.cuda.synchronize()
        return None
    return g.replay


def timed(run):
    if isinstance(run, tuple):                                  # (prepare, run): prepare is outside the timed window
        run[0]()
        run = run[1]
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3      # us


def rounds_of(forms, rounds):
    us = {k: [] for k in forms}
    for r in range(rounds + 1):                                 # alternating; round 0 is the warm-up
        for k, run in forms.items():
            v = timed(run)
            if r:
                us[k].append(v)
    return us


def fmt(v):
    return f"median {statistics.median(v):9.2f} us (min {min(v):.2f}, max {max(v):.2f})"


def build(model, dev):
    import bench
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import SD15_CONFIG, SDXL_CONFIG, build_unet, quantizable_layers
    cfg, latent = (SDXL_CONFIG, 128) if model == "sdxl" else (SD15_CONFIG, 64)
    unet = build_unet(dev, cfg=cfg)
    inp = example_inputs(2, latent, dev, seed=42, cfg=cfg)
    with torch.no_grad():
        ckpt = calibrate(unet, [inp])
    names = list(quantizable_layers(unet))
    act = {n: 8 for n in names if model == "sdxl" or n not in ("conv_in", "conv_out")}
    quantize_unet(unet, bench.Cfg({n: 8 for n in names}, act), ckpt, bos=True,
                  bos_dict=precompute_bos(unet, inp["encoder_hidden_states"]))
    return unet.set_fused(True), inp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--forward", default="sdxl", choices=("sdxl", "sd15", "none"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_freeu.py measures on the GPU"
    import mixdq_amd._C as C
    dev, cl = "cuda:0", torch.channels_last
    lines = [f"_C.freeu against the torch.fft chain, {a.reps} calls per graph, per call; floor = bytes read and written once at "
             "8 TB/s"]
    g = torch.Generator(device=dev).manual_seed(0)
    table = torch.tensor([[1.5, 0.9], [1.6, 0.2]], device=dev)
    for model, pairs in PAIRS.items():
        for B in (1, 2):
            for i, (c_h, c_s, L) in enumerate(pairs):
                hidden = (torch.randn(B, c_h, L, L, generator=g, device=dev) * 0.5 + 0.7).half().contiguous(memory_format=cl)
                skip = (torch.randn(B, c_s, L, L, generator=g, device=dev) * 0.5 + 0.7).half().contiguous(memory_format=cl)
                stage = i // 3
                b, s = table[stage].tolist()
                forms = {"launch": graphed(lambda: C.freeu(hidden, skip, table, stage), a.reps),
                         "chain": graphed(lambda: chain(hidden, skip, b, s), a.reps)}
                eager = forms["chain"] is None
                if eager:
                    forms["chain"] = lambda: [chain(hidden, skip, b, s) for _ in range(a.reps)]
                us = {k: [x / a.reps for x in v] for k, v in rounds_of(forms, a.rounds).items()}
                floor = 4 * B * L * L * (c_h + c_s) / HBM_BYTES_PER_S * 1e6
                lines.append(f"  {model} B={B} hidden {c_h} skip {c_s} {L}x{L}: launch {fmt(us['launch'])}; chain"
                             f"{' (eager)' if eager else ''} {fmt(us['chain'])}; floor {floor:.2f} us; "
                             f"chain / launch {statistics.median(us['chain']) / statistics.median(us['launch']):.1f}x")
    if a.forward != "none":
        unet, inp = build(a.forward, dev)
        forms = {}
        with torch.no_grad():
            for name, values in (("off", None), ("on", (0.9, 0.2, 1.5, 1.6)), ("all-ones", (1, 1, 1, 1))):
                unet.disable_freeu() if values is None else unet.enable_freeu(*values)
                replay = graphed(lambda: unet(**inp), 1)
                # the two FreeU graphs read ONE table (it lives as long as the UNet): each gets its values before its replay
                forms[name] = replay if values is None else ((lambda v=values: unet.enable_freeu(*v)), replay)
        us = rounds_of(forms, a.rounds)
        lines.append(f"whole fused W8A8 {a.forward} forward, batch 2 (a guided pair), one graph each:")
        lines += [f"  FreeU {k:8s} {fmt(v)}" for k, v in us.items()]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
