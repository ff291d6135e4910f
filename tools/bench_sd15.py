"""Step time of the SD 1.5 UNet (mixdq_amd.unet.SD15_CONFIG) at 512 px, hipGraph-timed with tools/bench_attn.py's timer.

    python tools/bench_sd15.py [--bs 1,2] [--repeats 3] [--reps 10] [--out profiles/sd15_bench.txt]

Four networks on the same box, in this order in one process, per batch size (1: LCM runs without guidance; 2: a guided
pair): stock PyTorch FP16; the module swap alone (quantize_unet: every Linear / Conv2d a W8A8 layer, the glue stock
PyTorch); the module swap + swap_glue=True; this project's own fused graph (set_fused).  Uniform W8A8 + BOS, synthetic
weights, calibrated on the batch-2 inputs.  Each figure is the time of one UNet forward inside a captured graph of
`--reps` forwards, after warm-up (3 eager calls, 10 untimed replays); `--repeats` re-measures every network, so the
spread of the tool on the box is in the output.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_attn import timed  # noqa: E402


class _Cfg:
    def __init__(self, w, a):
        self.w_config, self.a_config = w, a


def _slice(inp, n):
    return dict(sample=inp["sample"][:n].contiguous(), timestep=inp["timestep"],
                encoder_hidden_states=inp["encoder_hidden_states"][:n].contiguous(), added_cond_kwargs=None)


def _commit():
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        r = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=root, capture_output=True, text=True)
        return r.stdout.strip() or "unknown (no git metadata)"
    except OSError:
        return "unknown"


def _lib_sha16(C):
    """The hash of the kernel sources the LOADED library was built from (mixdq_amd/build.py embeds it)."""
    import ctypes
    try:
        fn = C._lib.mixdq_build_csrc_sha16
        fn.restype = ctypes.c_char_p
        return fn().decode()
    except (AttributeError, OSError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", default="1,2")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="forwards per captured graph")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sd15.py needs a GPU"
    from mixdq_amd import _C
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.nn.glue import swap_glue_modules, unswap_glue_modules
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import SD15_CONFIG, build_unet, quantizable_layers
    dev = torch.device("cuda:0")
    batches = [int(x) for x in a.bs.split(",")]
    unet = build_unet(dev, cfg=SD15_CONFIG)
    inputs2 = example_inputs(2, 64, dev, seed=42, cfg=SD15_CONFIG)
    inputs = {b: (inputs2 if b == 2 else _slice(inputs2, b) if b < 2
                  else example_inputs(b, 64, dev, seed=42, cfg=SD15_CONFIG)) for b in batches}
    res = {"tool": "bench_sd15", "network": "SD 1.5 UNet, 512 px (latent 64), uniform W8A8 + BOS, synthetic weights",
           "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "hip": torch.version.hip,
           "lib_csrc_sha16": _lib_sha16(_C),
           "commit": _commit(), "reps_per_graph": a.reps, "repeats": a.repeats, "ms_per_step": {}}

    def measure(key):
        for b in batches:
            inp = inputs[b]
            with torch.no_grad():
                ms = [round(timed(lambda: unet(**inp), reps=a.reps) / 1e3, 4) for _ in range(a.repeats)]
            res["ms_per_step"].setdefault(key, {})[f"bs{b}"] = ms
            print(f"# {key} bs{b}: {ms} ms", file=sys.stderr, flush=True)

    measure("fp16_torch")
    with torch.no_grad():
        ckpt = calibrate(unet, [inputs2])
    names = list(quantizable_layers(unet))
    quantize_unet(unet, _Cfg({n: 8 for n in names}, {n: 8 for n in names if n not in ("conv_in", "conv_out")}), ckpt,
                  bos=True, bos_dict=precompute_bos(unet, inputs2["encoder_hidden_states"]))
    del ckpt
    measure("module_swap")
    swap_glue_modules(unet)
    measure("module_swap_glue")
    unswap_glue_modules(unet)
    unet.set_fused(True)
    measure("fused_graph")
    best = {k: {b: min(v) for b, v in d.items()} for k, d in res["ms_per_step"].items()}
    res["best_ms"] = best
    res["speedup_vs_fp16"] = {k: {b: round(best["fp16_torch"][b] / v, 3) for b, v in d.items()}
                              for k, d in best.items() if k != "fp16_torch"}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_sd15.py: ms per UNet forward, hipGraph-timed; one list entry per repeat\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
