"""Time the CLIP vision encoder on one MI355X: the `_C.clip_patch_embed` launch against the torch chain it replaces
(FP16 normalise, conv2d, cat, add, layer_norm) at ViT-H/14's shape, batch 1 and 4; and a whole ViT-H forward against the
same network built from stock nn modules with scaled_dot_product_attention in FP16.  Synthetic weights.

    python tools/bench_vision.py [--rounds 7] [--reps 20] [--forward h|l|none] [--out profiles/vision_bench.txt]

Everything is timed from captured graphs (`reps` calls per graph, device events around one replay), the forms alternating
within a round after one warm-up round; medians with the rounds' min and max."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_freeu import fmt, graphed, rounds_of  # noqa: E402

HBM_BYTES_PER_S = 8.0e12        # MI355X peak
MFMA_F16_FLOPS = 2.5e15         # dense FP16 matrix peak


def chain(image_u8, mean, std, em, ln):
    """What stock PyTorch runs for the front of the tower, from the uint8 image, in FP16."""
    pv = (image_u8.half() / 255.0 - mean) / std
    x = em.patch_embedding(pv).flatten(2).transpose(1, 2)
    x = torch.cat([em.class_embedding.expand(len(x), 1, -1), x], dim=1) + em.position_embedding.weight
    return F.layer_norm(x, ln.weight.shape, ln.weight, ln.bias, ln.eps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--forward", default="h", choices=("h", "l", "none"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vision.py measures on the GPU"
    from mixdq_amd import vision as V
    from tests import vision_ref
    dev = "cuda:0"
    cfg = V.CLIP_VIT_L_CONFIG if a.forward == "l" else V.CLIP_VIT_H_CONFIG
    name = "ViT-L/14" if a.forward == "l" else "ViT-H/14"
    enc = V.build_vision_encoder(cfg, device=dev)
    vm, N, T = enc.vision_model, cfg["hidden_size"], (cfg["image_size"] // 14) ** 2
    mean, std = (torch.tensor(v, dtype=torch.float16, device=dev).view(1, 3, 1, 1) for v in (V.CLIP_MEAN, V.CLIP_STD))
    lines = [f"{torch.cuda.get_device_name(0)}; {a.reps} calls per graph, per call; {a.rounds} alternating rounds",
             f"the patch-embed launch against the torch FP16 chain (normalise, conv2d, cat, add, layer_norm), {name}, 224 px; floor = "
             "the larger of bytes once at 8 TB/s and the product's FLOPs at 2.5 PFLOP/s"]
    g = torch.Generator(device="cpu").manual_seed(0)
    with torch.no_grad():
        for B in (1, 4):
            image = torch.randint(0, 256, (B, 3, 224, 224), generator=g, dtype=torch.uint8).to(dev)
            forms = {"launch": graphed(lambda: enc_front(enc, image), a.reps),
                     "chain": graphed(lambda: chain(image, mean, std, vm.embeddings, vm.pre_layrnorm), a.reps)}
            us = {k: [x / a.reps for x in v] for k, v in rounds_of(forms, a.rounds).items()}
            nbytes = image.numel() + 2 * (N * 588 + (T + 1) * N + 3 * N + B * (T + 1) * N)
            floor = max(nbytes / HBM_BYTES_PER_S, 2.0 * B * T * 588 * N / MFMA_F16_FLOPS) * 1e6
            lines.append(f"  B={B} ({(T + 15) // 16 + 1} x {B} workgroups): launch {fmt(us['launch'])}; chain {fmt(us['chain'])}; "
                         f"floor {floor:.2f} us; chain / launch {statistics.median(us['chain']) / statistics.median(us['launch']):.2f}x")
        if a.forward != "none":
            stock = vision_ref.stock_encoder(cfg, enc.state_dict(), torch.float16, dev)
            for B in (1, 4):
                image = torch.randint(0, 256, (B, 3, 224, 224), generator=g, dtype=torch.uint8).to(dev)
                forms = {"ours": graphed(lambda: enc(image), 1),
                         "stock": graphed(lambda: stock((image.half() / 255.0 - mean) / std), 1)}
                us = rounds_of(forms, a.rounds)
                lines.append(f"  whole {name} forward B={B}, one graph each: ours {fmt(us['ours'])}; stock nn modules + SDPA, FP16 "
                             f"{fmt(us['stock'])}; stock / ours {statistics.median(us['stock']) / statistics.median(us['ours']):.2f}x")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def enc_front(enc, image):
    from mixdq_amd import _C
    vm = enc.vision_model
    return _C.clip_patch_embed(image, enc._norm(image.device, True), enc._derived()["patch"][0], vm.embeddings.class_embedding,
                               vm.embeddings.position_embedding.weight, vm.pre_layrnorm.weight, vm.pre_layrnorm.bias,
                               vm.pre_layrnorm.eps)


if __name__ == "__main__":
    main()
