"""What the 9-channel inpainting checkpoints cost: the split conv_in against a per-step torch.cat, against the 4-channel
blend, and the three new launches against torch.

    python tools/bench_inpaint9.py [--repeats 7] [--out profiles/inpaint9_bench.txt]

One box, one process, synthetic weights, uniform W8A8 + BOS, the fused graph:
  sampling   SDXL at 1024 px (latent 128), 4 euler_ancestral steps at batch 1.  `cond9`: Sampler.sample(cond=) on the
             9-channel UNet (conv_in split: its conditioning term computed once per call, outside the graph).
             `cat_in_graph`: the SAME UNet behind a wrapper whose forward is unet(torch.cat([x, cond], 1), ...) -- the
             drop-in form, the concatenation and the 9 -> 16 channel padding captured in every step.  `masked4`: the
             4-channel UNet's masked run, sample(init_latents=, mask=).  Alternating, `--repeats` times each after 2
             untimed runs; host clock from the call to a device synchronise behind it.
  cond_term  unet.cond_term(cond) alone, 20 calls per timed sample.
  inpaint    a whole Sampler.inpaint(composite=True) at 1024 px with the SDXL VAE: the 9-channel UNet (two encodes
             with strength, the mask ingest, the conditioning, a plain loop, decode, composite) against the 4-channel
             one (one encode, the masked loop, decode, composite), both with strength 0.5 -> 2 steps.
  ingest     _C.image_to_nhwc8_f16(x, mask) against from_uint8(x) * (mask < 0.5) at 1024 px, 20 calls per sample.
  dilate     _C.mask_dilate(mask, r) at 1024 x 1024, r = 6 and 32, against F.max_pool2d of the binarised mask
             (binarisation and the uint8 result included on both sides); results compared bit for bit.
The spread of a loop is (max - min) / median of its own samples.  Prints one JSON line per case."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_inpaint import _alternate, _Cfg  # noqa: E402
from tools.bench_sd15 import _commit, _lib_sha16  # noqa: E402


class _CatUNet:
    """The 9-channel UNet as a 4-channel one whose forward concatenates a static conditioning tensor per call."""
    cond_channels = 0

    def __init__(self, unet, cond):
        self.unet, self.cond = unet, cond

    def forward(self, sample, timestep, encoder_hidden_states, added_cond_kwargs=None):
        return self.unet.forward(torch.cat([sample, self.cond], dim=1), timestep, encoder_hidden_states,
                                 added_cond_kwargs)


def _record(lines, case, ms, med, spread, **extra):
    rec = {"case": case, "ms": ms, "median_ms": med, "min_ms": {k: min(v) for k, v in ms.items()}, "spread": spread}
    rec.update(extra)
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--tiny", action="store_true", help="the tiny UNet and VAE at latent 32 (a rehearsal, not a figure)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_inpaint9.py needs a GPU"
    import bench
    from mixdq_amd import Sampler, _C, cfgs
    from mixdq_amd import vae as V
    from mixdq_amd.calib import calibrate, precompute_bos
    from mixdq_amd.quantize_sdxl import example_inputs, quantize_unet
    from mixdq_amd.unet import build_unet, quantizable_layers
    dev = torch.device("cuda:0")
    head = {"tool": "bench_inpaint9", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
            "hip": torch.version.hip, "lib_csrc_sha16": _lib_sha16(_C), "commit": _commit(), "repeats": a.repeats,
            "unit": "ms per call, host clock to device synchronise"}
    lines = [json.dumps(head)]
    print(lines[0], flush=True)
    tiny_cfg = dict(bench.TINY_CFG, block_out_channels=(64, 128, 256), head_dim=64)
    L = 32 if a.tiny else 128
    tag = "tiny" if a.tiny else "sdxl_1024px"

    def make_unet(in_channels):
        cfg = dict(tiny_cfg, in_channels=in_channels) if a.tiny else dict(in_channels=in_channels)
        unet = build_unet(dev, cfg=cfg)
        inputs2 = example_inputs(2, L, dev, in_channels=in_channels, seed=42)
        ckpt = calibrate(unet, [inputs2])
        if a.tiny:
            names = list(quantizable_layers(unet))
            w_cfg, a_cfg = {n: 8 for n in names}, {n: 8 for n in names if n not in ("conv_in", "conv_out")}
        else:
            w_cfg, a_cfg = cfgs.load("weight/uniform_8"), cfgs.load("act/act_8.00")
        quantize_unet(unet, _Cfg(w_cfg, a_cfg), ckpt, bos=True,
                      bos_dict=precompute_bos(unet, inputs2["encoder_hidden_states"]))
        return unet.set_fused(True)

    unet9, unet4 = make_unet(9), make_unet(4)
    assert unet9.cond_channels == 5 and not getattr(unet9.conv_in, "valid_for_acceleration", False)
    n_steps = 4
    inp = example_inputs(1, L, dev, seed=7)
    ehs, added = inp["encoder_hidden_states"], inp["added_cond_kwargs"]
    gen = torch.Generator(device="cpu").manual_seed(11)
    noise = torch.randn(1, 4, L, L, generator=gen).to(dev)
    sn = torch.randn(n_steps, 1, 4, L, L, generator=gen).to(dev)
    z = (torch.randn(1, 4, L, L, generator=gen) * 0.13025).to(dev)
    mask = torch.zeros(1, L, L, device=dev)
    mask[:, L // 4:3 * L // 4, L // 4:3 * L // 4] = 1.0
    zm = (torch.randn(1, L, L, 4, generator=gen) * 0.13025).to(dev).permute(0, 3, 1, 2)
    cond = _C.inpaint_cond(mask, zm)

    # ---- sampling: the split conv_in against the concatenation in the graph and against the 4-channel blend
    sm9, sm4 = Sampler(unet9, "euler_ancestral", n_steps), Sampler(unet4, "euler_ancestral", n_steps)
    smcat = Sampler(_CatUNet(unet9, cond[:, :5].contiguous(memory_format=torch.channels_last)), "euler_ancestral", n_steps)
    loops = {"cond9": lambda: sm9.sample(noise, ehs, added, sn, cond=cond),
             "cat_in_graph": lambda: smcat.sample(noise, ehs, added, sn),
             "masked4": lambda: sm4.sample(noise, ehs, added, sn, init_latents=z, mask=mask)}
    ms, med, spread, outs = _alternate(loops, a.repeats, dev)
    d = (outs["cond9"] - outs["cat_in_graph"]).abs()
    _record(lines, f"{tag}_euler_ancestral_4step_bs1", ms, med, spread,
            cond9_minus_cat_ms=round(med["cond9"] - med["cat_in_graph"], 4),
            cond9_over_cat=round(med["cond9"] / med["cat_in_graph"], 4),
            cond9_over_masked4=round(med["cond9"] / med["masked4"], 4),
            latents_finite=bool(torch.isfinite(outs["cond9"]).all() and torch.isfinite(outs["cat_in_graph"]).all()),
            split_vs_cat_latents_max_abs=float(d.max()), split_vs_cat_latents_mean_abs=float(d.mean()),
            latents_rms=float(outs["cat_in_graph"].pow(2).mean().sqrt()))

    # ---- cond_term alone
    ms, med, spread, _ = _alternate({"cond_term": lambda: unet9.cond_term(cond)}, a.repeats, dev, calls=20)
    _record(lines, f"{tag}_cond_term", ms, med, spread, calls_per_sample=20)
    del smcat

    # ---- a whole inpaint()
    S = 8 * L
    vcfg = dict(V.VAE_SDXL_CONFIG, block_out_channels=(32, 64, 128, 512), layers_per_block=1, norm_num_groups=8) \
        if a.tiny else V.VAE_SDXL_CONFIG
    enc, dec = V.build_vae_encoder(vcfg, seed=11, device=dev), V.build_vae_decoder(vcfg, seed=11, device=dev)
    pixels = torch.randint(0, 256, (1, 3, S, S), generator=gen, dtype=torch.uint8).to(dev)
    m8 = torch.zeros(1, S, S, dtype=torch.uint8, device=dev)
    m8[:, S // 4:3 * S // 4, S // 4:3 * S // 4] = 255
    loops = {"inpaint9": lambda: sm9.inpaint(enc, dec, pixels, m8, noise, ehs, added, strength=0.5,
                                           step_noise=sn, composite=True),
             "inpaint4": lambda: sm4.inpaint(enc, dec, pixels, m8, noise, ehs, added, strength=0.5,
                                           step_noise=sn, composite=True)}
    ms, med, spread, outs = _alternate(loops, a.repeats, dev)
    outside = (m8 < 128)[:, None].expand_as(pixels)
    _record(lines, f"{tag}_inpaint_strength0.5_composite", ms, med, spread,
            inpaint9_over_inpaint4=round(med["inpaint9"] / med["inpaint4"], 4),
            outside_is_the_input=bool(all(torch.equal(outs[k][1][outside], pixels[outside]) for k in outs)))
    del sm9, sm4, unet9, unet4, enc, dec
    torch.cuda.empty_cache()

    # ---- the blanked ingest against torch
    mf = (m8.float() / 255.0)[:, None]
    loops = {"image_to_nhwc8_f16_masked": lambda: _C.image_to_nhwc8_f16(pixels, mf),
             "torch": lambda: V.from_uint8(pixels) * (mf < 0.5)}
    ms, med, spread, outs = _alternate(loops, a.repeats, dev, calls=20)
    _record(lines, f"blanked_ingest_{S}px", ms, med, spread, calls_per_sample=20,
            kernel_over_torch=round(med["image_to_nhwc8_f16_masked"] / med["torch"], 4),
            equal_values=bool(torch.equal(outs["image_to_nhwc8_f16_masked"][:, :3], outs["torch"])))

    # ---- the mask growth against max_pool2d
    big = (torch.rand(1, 1024, 1024, generator=gen) < 0.001).to(torch.uint8).to(dev) * 255
    for r in (6, 32):
        loops = {"mask_dilate": lambda: _C.mask_dilate(big, r),
                 "max_pool2d": lambda: (F.max_pool2d((big >= 128).float()[:, None], 2 * r + 1, 1, r)[:, 0] * 255
                                        ).to(torch.uint8)}
        ms, med, spread, outs = _alternate(loops, a.repeats, dev, calls=20)
        _record(lines, f"mask_dilate_1024px_r{r}", ms, med, spread, calls_per_sample=20,
                kernel_over_torch=round(med["mask_dilate"] / med["max_pool2d"], 4),
                bit_equal=bool(torch.equal(outs["mask_dilate"], outs["max_pool2d"])))
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_inpaint9.py: the 9-channel inpainting path -- split conv_in against torch.cat in the "
                    "graph and the 4-channel blend; cond_term; a whole inpaint(); the blanked ingest and the mask growth "
                    "against torch\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
