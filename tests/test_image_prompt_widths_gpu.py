"""GPU tests of the image-prompt chain at the widths that ship, two layers deep: the CLIP vision encoder as ViT-L/14 and
ViT-H/14 (hidden 1024 / 1280, 16 heads of 64 / 80, 257 tokens) and the IP-Adapter Plus Resampler as the SD 1.5 and SDXL
"plus" checkpoints configure it (dim 768 / 1280, 12 / 20 heads over 257 + 16 keys), each against the same network from
stock torch modules (tests/vision_ref.py, tests/resampler_ref.py) under the project's rule, and the two joined."""
import math

import pytest
import torch

from mixdq_amd.ip_adapter import RESAMPLER_PLUS_SD15, RESAMPLER_PLUS_SDXL, Resampler
from tests import resampler_ref, vision_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEPTH = 2


def vit_cfg(name):
    from mixdq_amd import vision as V
    return dict({"L": V.CLIP_VIT_L_CONFIG, "H": V.CLIP_VIT_H_CONFIG}[name], num_hidden_layers=DEPTH)


def ulp_floor(truth):
    return 2.0 ** (math.floor(math.log2(truth.abs().max().item())) - 10)


@pytest.mark.parametrize("name", ("L", "H"))
def test_encoder_at_shipped_widths(C, name):
    """tests/test_vision_gpu.py test_encoder_vs_the_stock_network's rule, per output: max |ours - fp32| <= max(1.5 x max
    |stock fp16 - fp32|, one FP16 ulp of the output range); the FP32 network runs on the CPU.  One 224-px image: 257
    tokens, patch embed at MAXT 16 / 20, linear_f16 at K = 1024 / 1280 / 4096 / 5120 with its activation and residual
    epilogues.  Then a graph: captured on the first image, replayed on a second and on the first again."""
    from mixdq_amd import vision as V
    from mixdq_amd.quantize_sdxl import hip_graph_opt
    cfg = vit_cfg(name)
    enc = V.build_vision_encoder(cfg, seed=11, device=DEV)
    images = torch.randint(0, 256, (2, 3, 224, 224), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).to(DEV)
    first, second = images[:1], images[1:]
    ours = enc(first)
    c = cfg["hidden_size"]
    assert tuple(ours.image_embeds.shape) == (1, cfg["projection_dim"])
    assert tuple(ours.last_hidden_state.shape) == tuple(ours.penultimate.shape) == (1, 257, c)
    pv = vision_ref.pixel_values(first, V.CLIP_MEAN, V.CLIP_STD)
    ref = vision_ref.stock_encoder(cfg, enc.state_dict(), torch.float32, "cpu")(pv)
    stock16 = vision_ref.stock_encoder(cfg, enc.state_dict(), torch.float16, DEV)(pv.half().to(DEV))
    for field, o, r, s16 in zip(ours._fields, ours, ref, stock16):
        assert o.dtype == torch.float16 and bool(torch.isfinite(o).all())
        err_ours, err_stock = ((x.float().cpu() - r).abs().max().item() for x in (o, s16))
        amax, ulp = r.abs().max().item(), ulp_floor(r)
        bound = max(1.5 * err_stock, ulp)
        print(f"vision ViT-{name} x {DEPTH} layers {field}: max |ref| {amax:.4f}, max err ours {err_ours:.3e}, stock fp16 "
              f"{err_stock:.3e}, ulp floor {ulp:.3e}, err / bound {err_ours / bound:.3f}")
        assert amax > 1e-2 and err_ours <= bound, field
    eager = [tuple(o.clone() for o in enc(im)) for im in (first, second)]
    assert not torch.equal(eager[0][0], eager[1][0])
    graphed = hip_graph_opt(V.build_vision_encoder(cfg, seed=11, device=DEV))
    for im, want in ((first, eager[0]), (second, eager[1]), (first, eager[0])):
        assert all(torch.equal(a, b) for a, b in zip(graphed(im), want))
    assert len(graphed.forward._cached) == 1


PLUS = {"sd15": dict(num_queries=16, output_dim=768, **dict(RESAMPLER_PLUS_SD15, depth=DEPTH)),
        "sdxl": dict(num_queries=16, output_dim=2048, **dict(RESAMPLER_PLUS_SDXL, depth=DEPTH))}


def plus_resampler(which, seed=5):
    """tests/test_resampler_gpu.py small_resampler's recipe at a shipped configuration; FP32 on the CPU."""
    torch.manual_seed(seed)
    rs = Resampler(**PLUS[which])
    with torch.no_grad():
        for _, p in rs.named_parameters():                       # LayerNorms that do something
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape))
    return rs.eval()


@pytest.fixture(scope="module", params=("sd15", "sdxl"))
def plus(request):
    """The FP32 truth on the CPU once per configuration, from the FP16 weights and the FP16 hidden [2, 257, 1280] upcast
    (what FP16 storage costs is no part of the comparison): both images, and the first on its own."""
    which = request.param
    rs = plus_resampler(which).half()
    heads = PLUS[which]["heads"]
    hidden = torch.randn(2, 257, 1280, generator=torch.Generator().manual_seed(257)).half()
    sd = {k: v.float() for k, v in rs.state_dict().items()}
    truth = {2: resampler_ref.forward(sd, hidden.float(), heads=heads, depth=DEPTH),
             1: resampler_ref.forward(sd, hidden[:1].float(), heads=heads, depth=DEPTH)}
    return dict(which=which, heads=heads, rs=rs.to(DEV), hidden=hidden.to(DEV), truth=truth)


def within_the_rule(tag, ours, stock, truth):
    err_ours, err_stock = ((x.float().cpu() - truth).abs().max().item() for x in (ours, stock))
    ulp = ulp_floor(truth)
    bound = max(1.5 * err_stock, ulp)
    print(f"Resampler {tag}: ours {err_ours:.3e}, stock fp16 {err_stock:.3e}, ulp floor {ulp:.3e}, "
          f"err / bound {err_ours / bound:.3f}")
    return bool(torch.isfinite(ours).all()) and err_ours <= bound


def test_resampler_at_shipped_widths_one_image(C, plus):
    """16 rows: every `_linear` call is the skinny launch.  tests/test_resampler_gpu.py's rule; then the device kernels
    of one forward: 5 * depth + 5 of this library's, `depth` of them the perceiver kernel, as the docstring says."""
    from torch.profiler import ProfilerActivity, profile
    rs, hd = plus["rs"], plus["hidden"][:1]
    assert rs._fast(hd)
    ours = rs(hd)
    assert tuple(ours.shape) == (1, 16, PLUS[plus["which"]]["output_dim"])
    stock = resampler_ref.forward(rs.state_dict(), hd, heads=plus["heads"], depth=DEPTH)
    assert within_the_rule(f"{plus['which']} B 1", ours, stock, plus["truth"][1])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        rs(hd)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
             and "Memcpy" not in e.name and "Memset" not in e.name]
    mine = [n for n in names if "mixdq" in n]
    assert len(mine) == 5 * DEPTH + 5, mine
    assert sum("attn_perceiver_kernel" in n for n in mine) == DEPTH
    assert sum("linear_skinny_kernel" in n for n in mine) == 4 * DEPTH + 1


def test_resampler_at_shipped_widths_two_images(C, plus):
    """32 rows: `_linear` sends the LayerNorm forms and the weights above 768 x 3072 to layernorm_quantize + linear_f16.
    Those sum in another order than the skinny launch, so each image's block is held to the rule, not to the bits of the
    one-image run."""
    rs, hd = plus["rs"], plus["hidden"]
    assert rs._fast(hd)
    ours = rs(hd)
    stock = resampler_ref.forward(rs.state_dict(), hd, heads=plus["heads"], depth=DEPTH)
    assert within_the_rule(f"{plus['which']} B 2", ours, stock, plus["truth"][2])
    for b in range(2):
        assert within_the_rule(f"{plus['which']} B 2 image {b}", ours[b], stock[b], plus["truth"][2][b])
    assert within_the_rule(f"{plus['which']} B 2 image 0 against the one-image truth", ours[:1], stock[:1], plus["truth"][1])


def test_encoder_feeds_the_resampler(C):
    """penultimate of the ViT-H encoder is read where the encoder left it: the same bits as from a copy."""
    from mixdq_amd import vision as V
    enc = V.build_vision_encoder(vit_cfg("H"), seed=11, device=DEV)
    rs = plus_resampler("sd15").half().to(DEV)
    image = torch.randint(0, 256, (1, 3, 224, 224), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).to(DEV)
    pen = enc(image).penultimate
    assert tuple(pen.shape) == (1, 257, 1280) and rs._fast(pen)
    got = rs(pen)
    assert torch.equal(got.view(torch.int16), rs(pen.clone()).view(torch.int16))
    assert tuple(got.shape) == (1, 16, 768) and bool(torch.isfinite(got).all())
