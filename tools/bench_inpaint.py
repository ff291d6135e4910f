"""What inpainting costs: a masked sampling run against an unmasked one, and the pixel composite against torch.

    python tools/bench_inpaint.py [--repeats 9] [--out profiles/inpaint_bench.txt]

One box, one process, synthetic weights:
  sampling   SDXL UNet at 1024 px (latent 128), uniform W8A8 + BOS, the fused graph, 4 euler_ancestral steps at batch
             1 on ONE Sampler: sample(noise, ...) (the plain graph: UNet + mixdq_sampler_step) against
             sample(noise, ..., init_latents=z, mask=m) (the second graph: UNet + mixdq_sampler_step_masked, plus
             three buffer copies per call), both the whole schedule from pure noise.  Alternating, `--repeats`
             times each after 2 untimed runs; timed on the host clock from the call to a device synchronise behind it.
  composite  vae.composite_uint8(decoded, original, mask) (one launch) against torch.where(mask_px, to_uint8(decoded),
             original) (eight torch operators) on a decode-shaped FP16 [1, 3, 1024, 1024] tensor, a uint8 original and a
             uint8 mask; 20 calls per timed sample, alternating; results compared bit for bit.
The spread of a loop is (max - min) / median of its own samples.  Prints one JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_sd15 import _commit, _lib_sha16  # noqa: E402


class _Cfg:
    def __init__(self, w, a):
        self.w_config, self.a_config = w, a


def _timed(fn, dev, calls=1):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(calls):
        out = fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0) / calls, out


def _alternate(loops, repeats, dev, calls=1):
    ms, outs = {k: [] for k in loops}, {}
    with torch.no_grad():
        for k, fn in loops.items():
            for _ in range(2):
                fn()
        for _ in range(repeats):
            for k, fn in loops.items():
                dt, outs[k] = _timed(fn, dev, calls)
                ms[k].append(round(dt, 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()}
    return ms, med, spread, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default="")
    ap.add_argument("--tiny", action="store_true", help="the tiny UNet at latent 32 instead (a rehearsal, not a figure)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_inpaint.py needs a GPU"
    import bench
    from mixdq_amd import Sampler, _C, cfgs
    from mixdq_amd import vae as V
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet, quantizable_layers
    dev = torch.device("cuda:0")
    head = {"tool": "bench_inpaint", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
            "hip": torch.version.hip, "lib_csrc_sha16": _lib_sha16(_C), "commit": _commit(), "repeats": a.repeats,
            "unit": "ms per call, host clock to device synchronise"}
    lines = [json.dumps(head)]
    print(lines[0], flush=True)

    # ---- sampling: masked against unmasked on one Sampler
    cfg, L = (dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64), 32) if a.tiny else (None, 128)
    unet = build_unet(dev, cfg=cfg)
    inputs2 = example_inputs(2, L, dev, seed=42, cfg=cfg)
    ckpt = calibrate(unet, [inputs2])
    if a.tiny:
        names = list(quantizable_layers(unet))
        w_cfg, a_cfg = {n: 8 for n in names}, {n: 8 for n in names if n not in ("conv_in", "conv_out")}
    else:
        w_cfg, a_cfg = cfgs.load("weight/uniform_8"), cfgs.load("act/act_8.00")
    quantize_unet(unet, _Cfg(w_cfg, a_cfg), ckpt, bos=True, bos_dict=precompute_bos(unet, inputs2["encoder_hidden_states"]))
    del ckpt
    unet.set_fused(True)
    n_steps = 4
    sm = Sampler(unet, "euler_ancestral", n_steps)
    inp = example_inputs(1, L, dev, seed=7, cfg=cfg)
    ehs, added = inp["encoder_hidden_states"], inp["added_cond_kwargs"]
    gen = torch.Generator(device="cpu").manual_seed(11)
    noise = torch.randn(1, 4, L, L, generator=gen).to(dev)
    sn = torch.randn(n_steps, 1, 4, L, L, generator=gen).to(dev)
    z = (torch.randn(1, 4, L, L, generator=gen) * 0.13025).to(dev)
    mask = torch.zeros(1, L, L, device=dev)
    mask[:, L // 4:3 * L // 4, L // 4:3 * L // 4] = 1.0
    loops = {"unmasked": lambda: sm.sample(noise, ehs, added, sn),
             "masked": lambda: sm.sample(noise, ehs, added, sn, init_latents=z, mask=mask)}
    ms, med, spread, outs = _alternate(loops, a.repeats, dev)
    keep = (mask == 0)[:, None].expand_as(z)
    rec = {"case": ("tiny" if a.tiny else "sdxl_1024px") + "_euler_ancestral_4step_bs1", "ms": ms, "median_ms": med,
           "min_ms": {k: min(v) for k, v in ms.items()}, "spread": spread,
           "masked_minus_unmasked_ms": round(med["masked"] - med["unmasked"], 4),
           "masked_over_unmasked": round(med["masked"] / med["unmasked"], 4),
           "kept_region_is_the_image": bool(torch.equal(outs["masked"][keep], z[keep])),
           "latents_finite": bool(torch.isfinite(outs["masked"]).all())}
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    del sm, unet
    torch.cuda.empty_cache()

    # ---- the composite against torch
    S = 256 if a.tiny else 1024
    four = (torch.randn(1, S, S, 4, generator=gen) * 0.8).to(torch.float16).to(dev)
    decoded = four.permute(0, 3, 1, 2)[:, :3]                      # as VAEDecoder.decode returns it
    original = torch.randint(0, 256, (1, 3, S, S), generator=gen, dtype=torch.uint8).to(dev)
    m8 = torch.zeros(1, S, S, dtype=torch.uint8, device=dev)
    m8[:, S // 4:3 * S // 4, S // 4:3 * S // 4] = 255
    loops = {"composite_uint8": lambda: V.composite_uint8(decoded, original, m8),
             "torch_where": lambda: torch.where((m8 >= 128)[:, None], V.to_uint8(decoded), original)}
    ms, med, spread, outs = _alternate(loops, a.repeats, dev, calls=20)
    rec = {"case": f"composite_{S}px", "calls_per_sample": 20, "ms": ms, "median_ms": med,
           "min_ms": {k: min(v) for k, v in ms.items()}, "spread": spread,
           "composite_over_torch": round(med["composite_uint8"] / med["torch_where"], 4),
           "bit_equal": bool(torch.equal(outs["composite_uint8"], outs["torch_where"]))}
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_inpaint.py: a masked sampling run against an unmasked one on one Sampler; the pixel "
                    "composite against torch.where\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
