"""The vision encoder of mixdq_amd.vision restated: the patch-embed launch's arithmetic (include/mixdq_math.h
mixdq_clip_*) in numpy float64, and the whole network from stock torch modules, any dtype and device (transformers'
CLIPVisionModelWithProjection layer by layer; takes the state dict of a mixdq_amd.vision.VisionEncoder)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.text_ref import _MLP


def im2col(image):
    """[B, 3, 14 g, 14 g] -> [B, g * g, 588], k = (c * 14 + y) * 14 + x, patches in raster order."""
    B, C, S, _ = image.shape
    g = S // 14
    return image.reshape(B, C, g, 14, g, 14).transpose(0, 2, 4, 1, 3, 5).reshape(B, g * g, C * 196)


def embed(image, norm, weight, cls, pos):
    """-> (e FP16 [B, g * g + 1, N], acc float64 [B, g * g, N] the exact sums, mag = sum_k |pix * w| alike).
    pix = f16(f32(u * a_c + b_c)): the float64 product-sum of a uint8 / FP16 pixel is exact, so its FP32 rounding is
    the fma's.  e = f16(f16(acc) + pos[1 + p]); row 0 = f16(cls + pos[0]).  With integer inputs every step is exact."""
    a, b = (np.asarray(norm, np.float32).astype(np.float64)[:, i].reshape(1, 3, 1, 1) for i in (0, 1))
    pix = (image.astype(np.float64) * a + b).astype(np.float32).astype(np.float16)
    cols, w = im2col(pix).astype(np.float64), weight.reshape(weight.shape[0], -1).astype(np.float64)
    acc, mag = cols @ w.T, np.abs(cols) @ np.abs(w).T
    body = (acc.astype(np.float16).astype(np.float64) + pos[1:].astype(np.float64)).astype(np.float16)
    row0 = (cls.astype(np.float64) + pos[0].astype(np.float64)).astype(np.float16)
    return np.concatenate([np.broadcast_to(row0, (len(body), 1, len(row0))), body], axis=1), acc, mag


def layernorm(e, gamma, beta, eps):
    """float64 LayerNorm of FP16 rows -> (y float64, xhat, rstd [.., 1])."""
    e = e.astype(np.float64)
    d = e - e.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt((d * d).mean(-1, keepdims=True) + eps)
    return d * rstd * gamma.astype(np.float64) + beta.astype(np.float64), d * rstd, rstd


class _Attn(nn.Module):
    def __init__(self, c, heads):
        super().__init__()
        self.heads = heads
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = (nn.Linear(c, c) for _ in range(4))

    def forward(self, x):
        B, T, C = x.shape
        q, k, v = (f(x).view(B, T, self.heads, C // self.heads).transpose(1, 2)
                   for f in (self.q_proj, self.k_proj, self.v_proj))
        return self.out_proj(F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, C))


class _Layer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        c, eps = cfg["hidden_size"], cfg["layer_norm_eps"]
        self.layer_norm1, self.layer_norm2 = nn.LayerNorm(c, eps=eps), nn.LayerNorm(c, eps=eps)
        self.self_attn = _Attn(c, cfg["num_attention_heads"])
        self.mlp = _MLP(c, cfg["intermediate_size"], cfg["hidden_act"])

    def forward(self, x):
        x = x + self.self_attn(self.layer_norm1(x))
        return x + self.mlp(self.layer_norm2(x))


class StockVisionEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        c, p, eps = cfg["hidden_size"], cfg["patch_size"], cfg["layer_norm_eps"]
        vm = self.vision_model = nn.Module()
        vm.embeddings = nn.Module()
        vm.embeddings.class_embedding = nn.Parameter(torch.zeros(c))
        vm.embeddings.patch_embedding = nn.Conv2d(3, c, p, p, bias=False)
        vm.embeddings.position_embedding = nn.Embedding((cfg["image_size"] // p) ** 2 + 1, c)
        vm.pre_layrnorm, vm.post_layernorm = nn.LayerNorm(c, eps=eps), nn.LayerNorm(c, eps=eps)
        vm.encoder = nn.Module()
        vm.encoder.layers = nn.ModuleList([_Layer(cfg) for _ in range(cfg["num_hidden_layers"])])
        self.visual_projection = nn.Linear(c, cfg["projection_dim"], bias=False)

    @torch.no_grad()
    def forward(self, pixel_values):
        """(image_embeds, last_hidden_state, penultimate)"""
        vm, em = self.vision_model, self.vision_model.embeddings
        x = em.patch_embedding(pixel_values).flatten(2).transpose(1, 2)
        x = torch.cat([em.class_embedding.expand(len(x), 1, -1), x], dim=1) + em.position_embedding.weight
        x = pen = vm.pre_layrnorm(x)
        for layer in vm.encoder.layers:
            pen, x = x, layer(x)
        return self.visual_projection(vm.post_layernorm(x[:, 0])), x, pen


def stock_encoder(cfg, state_dict, dtype, device):
    """The stock network with `state_dict`'s weights (FP16 values, upcast exactly when dtype is wider)."""
    m = StockVisionEncoder(cfg)
    m.load_state_dict({k: v.detach().to("cpu", torch.float32) for k, v in state_dict.items()}, strict=True)
    return m.to(device=device, dtype=dtype).eval()


def pixel_values(image_u8, mean, std):
    """CLIPImageProcessor's rescale and normalise, FP32 on the CPU: (u / 255 - mean) / std."""
    m, s = (torch.tensor(v, dtype=torch.float32).view(1, 3, 1, 1) for v in (mean, std))
    return (image_u8.cpu().float() / 255.0 - m) / s
