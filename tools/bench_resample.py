"""What the resampling kernels cost, next to the torch operators one would use instead.

    python tools/bench_resample.py [--repeats 7] [--out profiles/resample_bench.txt]

One box, one process:
  resize     image.resize of a uint8 [1, 3, S, S] image, lanczos3, 1024 -> 512 and 512 -> 1024 (one launch), against
             F.interpolate(image.float(), mode='bicubic', antialias=True).round().clamp(0, 255).to(uint8) on the same
             tensor (torch has no Lanczos; its antialiased bicubic is the nearest operator, with 2/3 of the taps).
             20 calls per timed sample.  The results differ by the filters; the largest difference is printed.
  paste      image.paste of a decode-shaped FP16 [1, 3, 1024, 1024] tensor into the 1536 x 1536 window (256, 256,
             1792, 1792) of a uint8 [1, 3, 2048, 2048] original under a soft uint8 mask (one copy + one launch), against
             the torch chain: clone, F.interpolate(bicubic, antialias) of the decode, to_uint8, the blend in FP32,
             round, the slice assignment.  20 calls per timed sample.
  inpaint    Sampler.inpaint(crop=window, mask_blur=4) on a 1024 x 1024 photograph against Sampler.inpaint() on a
             model-sized image with composite=True: the tiny UNet (latent 32, 256 px) and a small VAE, 4 euler steps at
             strength 0.5, synthetic weights -- the difference is the image side (two resizes, the blur, the paste in
             place of the composite), which does not depend on the UNet's size.
Alternating, `--repeats` timed samples each after 2 untimed runs, on the host clock from the call to a device
synchronise behind it; the spread of a loop is (max - min) / median of its own samples.  One JSON line per case."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_inpaint import _alternate, _Cfg  # noqa: E402
from tools.bench_sd15 import _commit, _lib_sha16  # noqa: E402


def _record(case, ms, med, spread, ours, theirs, **extra):
    rec = {"case": case, "ms": ms, "median_ms": med, "min_ms": {k: min(v) for k, v in ms.items()}, "spread": spread,
           f"{ours}_over_{theirs}": round(med[ours] / med[theirs], 4)}
    rec.update(extra)
    return json.dumps(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resample.py needs a GPU"
    import bench
    from mixdq_amd import Sampler, _C
    from mixdq_amd import image as I
    from mixdq_amd import vae as V
    dev = torch.device("cuda:0")
    head = {"tool": "bench_resample", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
            "hip": torch.version.hip, "lib_csrc_sha16": _lib_sha16(_C), "commit": _commit(), "repeats": a.repeats,
            "unit": "ms per call, host clock to device synchronise"}
    lines = [json.dumps(head)]
    print(lines[0], flush=True)
    gen = torch.Generator(device="cpu").manual_seed(5)

    # ---- resize against F.interpolate
    for S, D in ((1024, 512), (512, 1024)):
        img = torch.randint(0, 256, (1, 3, S, S), generator=gen, dtype=torch.uint8).to(dev)
        loops = {"resize": lambda: I.resize(img, (D, D), None, "lanczos3"),
                 "torch": lambda: F.interpolate(img.float(), size=(D, D), mode="bicubic", antialias=True)
                 .round().clamp(0, 255).to(torch.uint8)}
        ms, med, spread, outs = _alternate(loops, a.repeats, dev, calls=20)
        diff = int((outs["resize"].int() - outs["torch"].int()).abs().max())
        lines.append(_record(f"resize_u8_3ch_{S}_to_{D}_lanczos3", ms, med, spread, "resize", "torch", calls_per_sample=20,
                             max_abs_difference_to_torch_bicubic=diff))
        print(lines[-1], flush=True)

    # ---- the paste against the torch chain
    four = (torch.randn(1, 1024, 1024, 4, generator=gen) * 0.8).to(torch.float16).to(dev)
    decoded = four.permute(0, 3, 1, 2)[:, :3]                      # as VAEDecoder.decode returns it
    original = torch.randint(0, 256, (1, 3, 2048, 2048), generator=gen, dtype=torch.uint8).to(dev)
    hard = torch.zeros(1, 2048, 2048, dtype=torch.uint8, device=dev)
    hard[:, 600:1500, 500:1600] = 255
    soft = I.blur_mask(hard, 8.0)
    x0, y0, x1, y1 = win = (256, 256, 1792, 1792)

    def torch_paste():
        out = original.clone()
        d = V.to_uint8(F.interpolate(decoded.float(), size=(y1 - y0, x1 - x0), mode="bicubic", antialias=True)
                       .to(torch.float16)).float()
        m = soft[:, None, y0:y1, x0:x1].float() / 255.0
        out[:, :, y0:y1, x0:x1] = (m * d + (1.0 - m) * out[:, :, y0:y1, x0:x1].float()).round().to(torch.uint8)
        return out
    loops = {"paste": lambda: I.paste(decoded, original, soft, win, "lanczos3", soft=True), "torch": torch_paste}
    ms, med, spread, outs = _alternate(loops, a.repeats, dev, calls=20)
    diff = int((outs["paste"].int() - outs["torch"].int()).abs().max())
    lines.append(_record("paste_1024_decode_into_1536_window_of_2048", ms, med, spread, "paste", "torch",
                         calls_per_sample=20, max_abs_difference_to_torch_bicubic=diff))
    print(lines[-1], flush=True)
    del four, decoded, original, hard, soft

    # ---- a whole cropped inpaint against a plain one at the same model size
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet, quantizable_layers
    cfg, L = dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64), 32
    unet = build_unet(dev, cfg=cfg)
    inputs2 = example_inputs(2, L, dev, seed=42, cfg=cfg)
    ckpt = calibrate(unet, [inputs2])
    names = list(quantizable_layers(unet))
    quantize_unet(unet, _Cfg({n: 8 for n in names}, {n: 8 for n in names if n not in ("conv_in", "conv_out")}), ckpt,
                  bos=True, bos_dict=precompute_bos(unet, inputs2["encoder_hidden_states"]))
    unet.set_fused(True)
    vcfg = dict(V.VAE_SDXL_CONFIG, block_out_channels=(32, 64, 128, 512), layers_per_block=1, norm_num_groups=8)
    enc, dec = V.build_vae_encoder(vcfg, seed=11, device=dev), V.build_vae_decoder(vcfg, seed=11, device=dev)
    sm = Sampler(unet, "euler", 4)
    inp = example_inputs(1, L, dev, seed=7, cfg=cfg)
    ehs, added = inp["encoder_hidden_states"], inp["added_cond_kwargs"]
    noise = torch.randn(1, 4, L, L, generator=gen).to(dev)
    P = 8 * L
    photo = torch.randint(0, 256, (1, 3, 1024, 1024), generator=gen, dtype=torch.uint8).to(dev)
    pmask = torch.zeros(1, 1024, 1024, dtype=torch.uint8, device=dev)
    pmask[:, 300:600, 350:700] = 255
    box = I.crop_region(I.mask_bbox(pmask)[0], (1024, 1024), (P, P), 32)
    small = torch.randint(0, 256, (1, 3, P, P), generator=gen, dtype=torch.uint8).to(dev)
    smask = torch.zeros(1, P, P, dtype=torch.uint8, device=dev)
    smask[:, P // 4:3 * P // 4, P // 4:3 * P // 4] = 255
    loops = {"cropped": lambda: sm.inpaint(enc, dec, photo, pmask, noise, ehs, added, strength=0.5, composite=True,
                                           crop=box, mask_blur=4),
             "plain": lambda: sm.inpaint(enc, dec, small, smask, noise, ehs, added, strength=0.5, composite=True)}
    ms, med, spread, outs = _alternate(loops, a.repeats, dev)
    lines.append(_record(f"inpaint_tiny_unet_{P}px_crop_{box[2] - box[0]}x{box[3] - box[1]}_of_1024", ms, med, spread,
                         "cropped", "plain", cropped_minus_plain_ms=round(med["cropped"] - med["plain"], 4),
                         box=list(box)))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_resample.py: resize and paste against the torch operators; a cropped inpaint against a "
                    "plain one\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
