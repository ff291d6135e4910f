"""IP-Adapter: image-prompt conditioning through decoupled cross-attention.

An adapter brings, per cross-attention of the UNet, a bias-free `to_k_ip` / `to_v_ip` pair that projects a few image
tokens to extra keys and values; the cross-attention becomes

    out = attn(q, K_text, V_text) + s * attn(q, K_ip, V_ip)

(diffusers' IPAdapterAttnProcessor2_0), which `SDXLUNet.forward(ip=IPState(...))` runs as ONE mixdq_attention_f16_ip
launch per layer.  The image keys and values do not change during a run: `IPAdapter.tokens` and `IPAdapter.kv` compute
them once per run, outside a captured graph.

Parameter names are the published checkpoint's: `image_proj.proj`, `image_proj.norm`, `ip_adapter.<i>.to_k_ip` /
`to_v_ip` with i = 2 n + 1, n counting the UNet's transformer blocks (one cross-attention each) in registration order:
down, mid, up.  diffusers is not available where this was written: that index rule is NOT verified against its loader.
The image embeddings come from mixdq_amd.vision (`vision(image).image_embeds`) or from the caller.
Not here: the Resampler of the "plus" adapters (pass its
[B, T, cross_dim] tokens to `kv`), ip_adapter_masks, FaceID's LoRA, quantized to_k_ip / to_v_ip, real weights.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from mixdq_amd import derived


class IPState:
    """What SDXLUNet.forward(ip=...) reads: `kv` -- per adapter (1 to 4) the [R, T_j, sum_l 2 C_l] tensor IPAdapter.kv
    returned, layer l's k | v at columns IPAdapter.offsets[l] (one row per sample row) -- and `scales`, FP32
    [layers, n_ip] on the sample's device: cross-attention l reads row l (per-block scales work), in the kernel."""

    def __init__(self, kv, scales):
        self.kv = list(kv)
        self.scales = scales


def cross_attention_dims(unet_cfg):
    """(cross_attention_dim, [C_l of every cross-attention in registration order]) of the UNet this config builds."""
    from mixdq_amd.unet import SDXLUNet, cross_attentions
    with torch.device("meta"):
        unet = SDXLUNet(unet_cfg)
    attns = cross_attentions(unet)
    return attns[0].to_k.in_features, [a.to_k.out_features for a in attns]


class _ImageProj(nn.Module):
    def __init__(self, clip_embed_dim, cross_dim, num_tokens):
        super().__init__()
        self.proj = nn.Linear(clip_embed_dim, num_tokens * cross_dim)
        self.norm = nn.LayerNorm(cross_dim)


class _IPLayer(nn.Module):
    def __init__(self, cross_dim, dim):
        super().__init__()
        self.to_k_ip = nn.Linear(cross_dim, dim, bias=False)
        self.to_v_ip = nn.Linear(cross_dim, dim, bias=False)


class IPAdapter(nn.Module):
    def __init__(self, unet_cfg, clip_embed_dim, num_tokens=4):
        super().__init__()
        self.cross_dim, self.dims = cross_attention_dims(unet_cfg)
        self.num_tokens = int(num_tokens)
        self.image_proj = _ImageProj(clip_embed_dim, self.cross_dim, self.num_tokens)
        self.ip_adapter = nn.ModuleDict({str(2 * n + 1): _IPLayer(self.cross_dim, c) for n, c in enumerate(self.dims)})
        self.offsets = [2 * sum(self.dims[:n]) for n in range(len(self.dims))]     # layer n: k at off, v at off + C_n

    def _fast(self, x):
        return x.is_cuda and x.dtype == torch.float16 and self.image_proj.proj.weight.dtype == torch.float16

    @torch.no_grad()
    def tokens(self, image_embeds):
        """image_embeds [B, clip_embed_dim] -> [B, num_tokens, cross_dim]: the projection (mixdq_linear_f16) and the
        LayerNorm with FP16 output the text encoders use; stock torch on the CPU or for other dtypes."""
        p = self.image_proj
        if not (torch.is_tensor(image_embeds) and image_embeds.dim() == 2
                and image_embeds.shape[1] == p.proj.in_features):
            raise RuntimeError(f"IPAdapter.tokens: image_embeds should be [B, {p.proj.in_features}]")
        if self._fast(image_embeds):
            from mixdq_amd import _C
            y = _C.linear_f16(image_embeds, p.proj.weight, p.proj.bias).reshape(-1, self.num_tokens, self.cross_dim)
            return _C.layernorm_quantize(y, p.norm.weight, p.norm.bias, p.norm.eps, [], want_f16=True)[1]
        return p.norm(p.proj(image_embeds).reshape(-1, self.num_tokens, self.cross_dim))

    def stacked_weight(self):
        """[sum_l 2 C_l, cross_dim]: every layer's to_k_ip then to_v_ip rows, through the version-keyed cache (rebuilt
        in place when a weight was written, so a captured reader keeps its address)."""
        ws = [w for n in range(len(self.dims)) for w in (self.ip_adapter[str(2 * n + 1)].to_k_ip.weight,
                                                         self.ip_adapter[str(2 * n + 1)].to_v_ip.weight)]
        return derived.derive(derived.holder_of(self), "ip_kv", ws, lambda old, *w: (torch.cat(w, dim=0),))[0]

    @torch.no_grad()
    def kv(self, tokens):
        """tokens [R, T, cross_dim] -> [R, T, sum_l 2 C_l]: ONE mixdq_linear_f16 launch against the row-stacked
        weight; layer l's keys are columns offsets[l] .. + C_l, its values the C_l columns behind them."""
        if not (torch.is_tensor(tokens) and tokens.dim() == 3 and tokens.shape[2] == self.cross_dim):
            raise RuntimeError(f"IPAdapter.kv: tokens should be [R, T, {self.cross_dim}]")
        w = self.stacked_weight()
        if self._fast(tokens):
            from mixdq_amd import _C
            return _C.linear_f16(tokens, w, None)
        return F.linear(tokens, w)

    def _apply(self, fn, recurse=True):                # a move or a dtype change: the stacked weight goes with it
        derived.drop(derived.holder_of(self))
        return super()._apply(fn, recurse)


def build_ip_adapter(unet_cfg, clip_embed_dim, num_tokens=4, device=None, dtype=torch.float16, seed=4343):
    """An IPAdapter for the UNet `unet_cfg` builds, with synthetic weights (deterministic in `seed`)."""
    if device is not None and torch.device(device).type == "meta":
        with torch.device("meta"):
            return IPAdapter(unet_cfg, clip_embed_dim, num_tokens)
    ad = IPAdapter(unet_cfg, clip_embed_dim, num_tokens)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in ad.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * (p.shape[1] ** -0.5))
            elif name.endswith("norm.weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    ad = ad.to(dtype=dtype)
    return (ad.to(device) if device is not None else ad).eval()
