"""The FP16 CLIP vision encoder (transformers' CLIPVisionModelWithProjection) on this library's kernels: an image in,
the IP-Adapter's image embeddings out.

    vision = build_vision_encoder(CLIP_VIT_H_CONFIG, device="cuda")     # synthetic weights; load_state_dict takes
    image = vision.preprocess(photo_u8)                                 # transformers' names
    latents = sampler.sample(..., ip_embeds=vision(image).image_embeds)

The front of the network -- image normalisation, the 14 x 14 / stride-14 patch convolution, the class token, the
position embedding and pre_layrnorm -- is ONE launch (mixdq_clip_patch_embed_f16, csrc/clip_vision.hip).  Each layer is
the text encoder's chain (mixdq_amd.text) with a self-attention that is not causal: mixdq_layernorm_quantize with its
FP16 output, ONE q|k|v mixdq_linear_f16, mixdq_attention_f16 on the three column slices (80-wide heads in ViT-H, 64-wide
in ViT-L), out_proj with the layer input as residual, LayerNorm, fc1 with the activation in its epilogue and fc2 with
the residual.  The only torch operators of a forward are views and one row copy (the class-token row); none waits for
the GPU, so `hip_graph_opt(vision)` captures it.

Not here: OpenCLIP bigG's tower (head width 104, which mixdq_attention_f16 does not serve: refused), quantized layers, and FP16 only.  A floating-point path with no
counterpart in the reference: held to tolerance against the same network built from stock torch modules
(tests/vision_ref.py).  DESIGN.md section 3.42.  `penultimate` is what the "plus" adapters' Resampler reads
(mixdq_amd.ip_adapter.Resampler).
"""
from collections import namedtuple

import torch
import torch.nn as nn

from mixdq_amd.derived import DerivedWeights
from mixdq_amd.text import ACTIVATIONS, ClipEncoder, _cat_qkv

# OpenCLIP ViT-H/14 (laion2B): the image encoder of every SD 1.5 IP-Adapter, ip-adapter_sdxl_vit-h and the "plus" ones.
CLIP_VIT_H_CONFIG = dict(hidden_size=1280, num_hidden_layers=32, num_attention_heads=16, intermediate_size=5120,
                         hidden_act="gelu", projection_dim=1024, image_size=224, patch_size=14, layer_norm_eps=1e-5)
# OpenAI CLIP ViT-L/14.
CLIP_VIT_L_CONFIG = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                         hidden_act="quick_gelu", projection_dim=768, image_size=224, patch_size=14, layer_norm_eps=1e-5)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)       # CLIPImageProcessor's image_mean / image_std
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

VisionEncoderOutput = namedtuple("VisionEncoderOutput", ["image_embeds", "last_hidden_state", "penultimate"])


def pixel_norm(mean=CLIP_MEAN, std=CLIP_STD):
    """[(a_c, b_c)] with (u / 255 - mean_c) / std_c == u * a_c + b_c, in float64 (the launch takes their FP32 roundings
    and computes f16(fma(u, a_c, b_c)) -- one FP32 rounding where the stock processor's rescale, subtract and divide
    make three)."""
    return [(1.0 / (255.0 * s), -m / s) for m, s in zip(mean, std)]


class ClipVisionEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        c, p = cfg["hidden_size"], cfg["patch_size"]
        self.class_embedding = nn.Parameter(torch.zeros(c))
        self.patch_embedding = nn.Conv2d(3, c, kernel_size=p, stride=p, bias=False)
        self.position_embedding = nn.Embedding((cfg["image_size"] // p) ** 2 + 1, c)


class ClipVisionTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        c, eps = cfg["hidden_size"], cfg["layer_norm_eps"]
        self.embeddings = ClipVisionEmbeddings(cfg)
        self.pre_layrnorm = nn.LayerNorm(c, eps=eps)            # (transformers' spelling)
        self.encoder = ClipEncoder(cfg)
        self.post_layernorm = nn.LayerNorm(c, eps=eps)


def _pack_patch(old, weight):
    from mixdq_amd import _C
    return (_C.clip_pack_patch_weight(weight, None if old is None else old[0]),)


class VisionEncoder(DerivedWeights, nn.Module):
    """A CLIPVisionModelWithProjection, parameter names as transformers'."""

    def __init__(self, cfg=None):
        super().__init__()
        from mixdq_amd import _C
        self.cfg = dict(CLIP_VIT_H_CONFIG if cfg is None else cfg)
        c, heads = self.cfg["hidden_size"], self.cfg["num_attention_heads"]
        width = c // heads if heads > 0 else 0
        if c != heads * width or width not in _C.ATTENTION_HEAD_DIMS:
            raise ValueError("VisionEncoder: head width %d (hidden_size %d / %d heads) is not one attention_f16 serves %r"
                             " -- OpenCLIP bigG's 104-wide heads are not supported" % (width, c, heads, _C.ATTENTION_HEAD_DIMS))
        if self.cfg["hidden_act"] not in ACTIVATIONS:
            raise ValueError("VisionEncoder: hidden_act should be one of %r" % (ACTIVATIONS,))
        size, patch = self.cfg["image_size"], self.cfg["patch_size"]
        if patch != _C.CLIP_PATCH or size % patch != 0 or not 1 <= size // patch <= _C.CLIP_MAX_GRID:
            raise ValueError("VisionEncoder: patch_size should be %d and image_size a multiple of it up to %d"
                             % (_C.CLIP_PATCH, _C.CLIP_PATCH * _C.CLIP_MAX_GRID))
        if c % 64 != 0 or c > _C.CLIP_MAX_N:
            raise ValueError("VisionEncoder: hidden_size should be a multiple of 64 up to %d" % _C.CLIP_MAX_N)
        self.heads, self.act = heads, self.cfg["hidden_act"]
        self.vision_model = ClipVisionTransformer(self.cfg)
        self.visual_projection = nn.Linear(c, self.cfg["projection_dim"], bias=False)
        self._norms = {}
        self._init_derived()

    def _derive(self):
        """The derived weights (lifecycle: DerivedWeights): layer index -> its q|k|v projection; "patch" -> the patch
        convolution's weight as the launch reads it."""
        d = {i: (layer.self_attn.qkv_sources(), _cat_qkv) for i, layer in enumerate(self.vision_model.encoder.layers)}
        d["patch"] = ((self.vision_model.embeddings.patch_embedding.weight,), _pack_patch)
        return d

    def _norm(self, device, pixels):
        """The launch's six normalisation values on `device`: CLIP's for pixels in 0..255, (1, 0) for pixel_values."""
        key = (str(device), pixels)
        if key not in self._norms:
            rows = pixel_norm() if pixels else [(1.0, 0.0)] * 3
            self._norms[key] = torch.tensor(rows, dtype=torch.float64).to(torch.float32).to(device)
        return self._norms[key]

    @staticmethod
    def _ln(norm, x):
        from mixdq_amd import _C
        return _C.layernorm_quantize(x, norm.weight, norm.bias, norm.eps, [], want_f16=True)[1]

    def _run_layer(self, layer, x, qkv):
        """text.ClipLayer.run with every query attending to every key."""
        from mixdq_amd import _C
        C = x.shape[-1]
        p = _C.linear_f16(self._ln(layer.layer_norm1, x), *qkv)
        att = _C.attention_f16(p[..., :C], p[..., C:2 * C], p[..., 2 * C:], self.heads)
        x = _C.linear_f16(att, layer.self_attn.out_proj.weight, layer.self_attn.out_proj.bias, _residual=x)
        h = _C.linear_f16(self._ln(layer.layer_norm2, x), layer.mlp.fc1.weight, layer.mlp.fc1.bias, _act=self.act)
        return _C.linear_f16(h, layer.mlp.fc2.weight, layer.mlp.fc2.bias, _residual=x)

    def preprocess(self, image_u8):
        """image_u8 [B, 3, H, W] (uint8, any strides, on the GPU) -> uint8 [B, 3, image_size, image_size]: the centred
        square of the short side resampled with the bicubic table, one mixdq_amd.image.resize launch.  This is
        crop-then-resize -- OUR definition: CLIPImageProcessor resizes the short side first and crops after, so its
        sampling phase can differ by a fraction of a source pixel.  Mean and std are not applied here: forward folds
        them into the patch-embed launch."""
        from mixdq_amd.image import resize
        H, W = image_u8.shape[-2:]
        s, size = min(H, W), self.cfg["image_size"]
        x0, y0 = (W - s) // 2, (H - s) // 2
        return resize(image_u8, (size, size), box=(x0, y0, x0 + s, y0 + s), filter="bicubic", out="u8")

    @torch.no_grad()
    def forward(self, image):
        """image [B, 3, image_size, image_size] on the GPU, any strides: uint8 pixels (normalised with CLIP's mean and
        std inside the first launch) or FP16 / FP32 `pixel_values` as CLIPImageProcessor makes them (taken as they are)
        -> VisionEncoderOutput of FP16 tensors: image_embeds [B, projection_dim] (visual_projection of post_layernorm
        of the class-token row: what sample(ip_embeds=) takes), last_hidden_state [B, g * g + 1, C] (the last layer's
        output, as transformers returns it: without post_layernorm) and penultimate (hidden_states[-2])."""
        from mixdq_amd import _C
        size = self.cfg["image_size"]
        if not (torch.is_tensor(image) and image.is_cuda and image.dim() == 4 and image.dtype in _C.IMAGE_DTYPES
                and tuple(image.shape[1:]) == (3, size, size)):
            raise RuntimeError("VisionEncoder.forward: image should be a [B, 3, %d, %d] uint8, FP16 or FP32 GPU tensor"
                               % (size, size))
        if any(p.dtype != torch.float16 for p in self.parameters()):          # (metadata only: no wait for the GPU)
            raise RuntimeError("VisionEncoder.forward: the encoder runs in FP16 (build_vision_encoder / .half())")
        vm = self.vision_model
        derived = self._derived()
        x = _C.clip_patch_embed(image, self._norm(image.device, image.dtype == torch.uint8), derived["patch"][0],
                                vm.embeddings.class_embedding, vm.embeddings.position_embedding.weight,
                                vm.pre_layrnorm.weight, vm.pre_layrnorm.bias, vm.pre_layrnorm.eps)
        penultimate = x
        for i, layer in enumerate(vm.encoder.layers):
            penultimate = x
            x = self._run_layer(layer, x, derived[i])
        pooled = self._ln(vm.post_layernorm, x[:, 0].contiguous())
        return VisionEncoderOutput(_C.linear_f16(pooled, self.visual_projection.weight, None), x, penultimate)


def state_dict_names(cfg=None):
    """(name, shape) of every parameter of transformers' CLIPVisionModelWithProjection with this config, written out
    from the layer list rather than read off the modules."""
    cfg = CLIP_VIT_H_CONFIG if cfg is None else cfg
    c, inter, p = cfg["hidden_size"], cfg["intermediate_size"], cfg["patch_size"]
    out = [("vision_model.embeddings.class_embedding", (c,)),
           ("vision_model.embeddings.patch_embedding.weight", (c, 3, p, p)),
           ("vision_model.embeddings.position_embedding.weight", ((cfg["image_size"] // p) ** 2 + 1, c))]
    lin = lambda n, o, i: [(n + ".weight", (o, i)), (n + ".bias", (o,))]
    norm = lambda n: [(n + ".weight", (c,)), (n + ".bias", (c,))]
    out += norm("vision_model.pre_layrnorm")
    for i in range(cfg["num_hidden_layers"]):
        pre = f"vision_model.encoder.layers.{i}."
        for s in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out += lin(pre + "self_attn." + s, c, c)
        out += norm(pre + "layer_norm1")
        out += lin(pre + "mlp.fc1", inter, c) + lin(pre + "mlp.fc2", c, inter)
        out += norm(pre + "layer_norm2")
    out += norm("vision_model.post_layernorm")
    out.append(("visual_projection.weight", (cfg["projection_dim"], c)))
    return out


def parameter_count(cfg=None) -> int:
    n = 0
    for _, shape in state_dict_names(cfg):
        k = 1
        for d in shape:
            k *= d
        n += k
    return n


def build_vision_encoder(cfg=None, seed: int = 42, device=None, dtype=torch.float16) -> VisionEncoder:
    """An encoder with synthetic weights: randn * 0.02 per linear layer and the patch convolution
    (init_synthetic_weights, as build_unet's), per embedding table and the class token, LayerNorm weights 1 + randn * 0.1
    and biases randn * 0.1; FP16, eval."""
    from mixdq_amd.unet import init_synthetic_weights
    enc = VisionEncoder(cfg)
    with torch.no_grad():
        init_synthetic_weights(enc, seed)
        for idx, (name, mod) in enumerate(enc.named_modules()):
            g = torch.Generator(device="cpu").manual_seed(seed + 100003 + idx)
            if isinstance(mod, nn.Embedding):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * 0.02)
            elif isinstance(mod, nn.LayerNorm):
                mod.weight.copy_(1 + torch.randn(mod.weight.shape, generator=g) * 0.1)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
            elif isinstance(mod, ClipVisionEmbeddings):
                mod.class_embedding.copy_(torch.randn(mod.class_embedding.shape, generator=g) * 0.02)
    enc = enc.to(dtype=dtype)
    if device is not None:
        enc = enc.to(device)
    return enc.eval()


if __name__ == "__main__":
    for _name, _cfg in (("CLIP_VIT_H_CONFIG", CLIP_VIT_H_CONFIG), ("CLIP_VIT_L_CONFIG", CLIP_VIT_L_CONFIG)):
        print(f"{_name}: {parameter_count(_cfg):,} parameters")
