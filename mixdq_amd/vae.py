"""The FP16 VAE decoder (diffusers' AutoencoderKL.decode) on this library's kernels: latents in, image out.

    vae = build_vae_decoder(VAE_SDXL_CONFIG).cuda()          # synthetic weights; load_state_dict takes diffusers' names
    image = vae.decode(latents)                              # [B, 4, h, w] FP32 / FP16 -> FP16 [B, 3, 8h, 8w]
    pixels = to_uint8(image)

Every layer runs channels-last in FP16 on the C-ABI library: mixdq_conv2d_f16 (the residual of a ResNet block folded
into its second conv, `Upsample2D`'s nearest 2x folded into the conv's gather: MIXDQ_FLAG_UPSAMPLE2X),
mixdq_groupnorm_silu_quantize with its FP16 output, mixdq_linear_f16 (one q|k|v projection, N = 3C) and
mixdq_attention_f16 at head width 512 reading the column slices.  The only torch operators of a decode are the dtype /
layout conversion of the 4-channel input and views; `hip_graph_opt(vae)` captures it.

This is a floating-point path with no counterpart in the reference (which reaches the VAE through diffusers'
pipeline): it is held to tolerance against the same network built from stock torch modules (tests/vae_ref.py).
DESIGN.md section 3.23.
"""
from collections import OrderedDict

import torch
import torch.nn as nn

VAE_SDXL_CONFIG = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4,
                       out_channels=3, norm_num_groups=32, scaling_factor=0.13025)
VAE_SD15_CONFIG = dict(VAE_SDXL_CONFIG, scaling_factor=0.18215)
GN_EPS = 1e-6


class VaeResnetBlock(nn.Module):
    def __init__(self, cin, cout, groups):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, cin, eps=GN_EPS)
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1)
        self.norm2 = nn.GroupNorm(groups, cout, eps=GN_EPS)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)

    def run(self, vae, x):
        from mixdq_amd import _C
        h = _C.conv2d_f16(vae._gn(self.norm1, x, True), self.conv1.weight, self.conv1.bias, 1, 1)
        h = vae._gn(self.norm2, h, True)
        if hasattr(self, "conv_shortcut"):
            x = _C.conv2d_f16(x, self.conv_shortcut.weight, self.conv_shortcut.bias, 1, 0)
        return _C.conv2d_f16(h, self.conv2.weight, self.conv2.bias, 1, 1, _residual=x)


class VaeAttention(nn.Module):
    """diffusers' Attention as the VAE's mid block uses it: one head as wide as the block, a residual connection."""

    def __init__(self, c, groups):
        super().__init__()
        self.group_norm = nn.GroupNorm(groups, c, eps=GN_EPS)
        self.to_q, self.to_k, self.to_v = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)
        self.to_out = nn.ModuleList([nn.Linear(c, c)])

    def qkv(self):
        """to_q | to_k | to_v as ONE [3C, C] projection."""
        return (torch.cat([self.to_q.weight, self.to_k.weight, self.to_v.weight]).contiguous(),
                torch.cat([self.to_q.bias, self.to_k.bias, self.to_v.bias]).contiguous())

    def run(self, vae, x):
        from mixdq_amd import _C
        B, C, H, W = x.shape
        w_qkv, b_qkv = vae._derived()["qkv"]
        rows = x.permute(0, 2, 3, 1).reshape(B, H * W, C)               # NHWC rows are the tokens: a view
        hn = vae._gn(self.group_norm, x, False).permute(0, 2, 3, 1).reshape(B, H * W, C)
        qkv = _C.linear_f16(hn, w_qkv, b_qkv)
        att = _C.attention_f16(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], 1)
        out = _C.linear_f16(att, self.to_out[0].weight, self.to_out[0].bias, _residual=rows)
        return out.view(B, H, W, C).permute(0, 3, 1, 2)


class VaeMidBlock(nn.Module):
    def __init__(self, c, groups):
        super().__init__()
        self.attentions = nn.ModuleList([VaeAttention(c, groups)])
        self.resnets = nn.ModuleList([VaeResnetBlock(c, c, groups), VaeResnetBlock(c, c, groups)])

    def run(self, vae, x):
        x = self.resnets[0].run(vae, x)
        x = self.attentions[0].run(vae, x)
        return self.resnets[1].run(vae, x)


class VaeUpsample(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, padding=1)


class VaeUpBlock(nn.Module):
    def __init__(self, cin, cout, n_resnets, groups, add_up):
        super().__init__()
        self.resnets = nn.ModuleList([VaeResnetBlock(cin if i == 0 else cout, cout, groups) for i in range(n_resnets)])
        if add_up:
            self.upsamplers = nn.ModuleList([VaeUpsample(cout)])

    def run(self, vae, x):
        from mixdq_amd import _C
        for r in self.resnets:
            x = r.run(vae, x)
        if hasattr(self, "upsamplers"):
            conv = self.upsamplers[0].conv      # the conv reads pixel (y >> 1, x >> 1): no upsampled tensor
            x = _C.conv2d_f16(x, conv.weight, conv.bias, 1, 1, _upsample2x=True)
        return x


class VaeDecoderNet(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        ch, g = tuple(cfg["block_out_channels"]), cfg["norm_num_groups"]
        self.conv_in = nn.Conv2d(cfg["latent_channels"], ch[-1], 3, padding=1)
        self.mid_block = VaeMidBlock(ch[-1], g)
        rev = ch[::-1]
        self.up_blocks = nn.ModuleList([
            VaeUpBlock(rev[max(i - 1, 0)], rev[i], cfg["layers_per_block"] + 1, g, i != len(rev) - 1)
            for i in range(len(rev))])
        self.conv_norm_out = nn.GroupNorm(g, ch[0], eps=GN_EPS)
        self.conv_out = nn.Conv2d(ch[0], cfg.get("out_channels", 3), 3, padding=1)


class VAEDecoder(nn.Module):
    """post_quant_conv + decoder of an AutoencoderKL, parameter names as diffusers'."""

    def __init__(self, cfg=None):
        super().__init__()
        self.cfg = dict(VAE_SDXL_CONFIG if cfg is None else cfg)
        lc = self.cfg["latent_channels"]
        self.post_quant_conv = nn.Conv2d(lc, lc, 1)
        self.decoder = VaeDecoderNet(self.cfg)
        self.scaling_factor = float(self.cfg["scaling_factor"])
        self._cache = None         # tensors derived from the weights (rebuilt after a load or a move)
        self._gn_ws = {}           # GroupNorm workspaces, one per (shape, device)

    # ---- derived weights ------------------------------------------------------------------------------------
    def padded_conv_out(self):
        """conv_out's weight / bias padded with zero output channels to a multiple of four (3 -> 4), the width the MFMA
        tiles take; decode() returns the first `out_channels` of that conv."""
        w, b = self.decoder.conv_out.weight, self.decoder.conv_out.bias
        k = w.shape[0]
        k4 = (k + 3) // 4 * 4
        w4 = torch.zeros((k4,) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)
        b4 = torch.zeros(k4, dtype=b.dtype, device=b.device)
        w4[:k], b4[:k] = w.detach(), b.detach()
        return w4.contiguous(memory_format=torch.channels_last), b4

    def scaled_post_quant_conv(self):
        """post_quant_conv on z / scaling_factor == the conv with weight / scaling_factor on z (the division is done
        once, in FP32, on the 4 x 4 weight; the bias is untouched)."""
        w = self.post_quant_conv.weight.detach()
        return ((w.float() / self.scaling_factor).to(w.dtype).contiguous(memory_format=torch.channels_last),
                self.post_quant_conv.bias.detach())

    @torch.no_grad()
    def _derived(self):
        if self._cache is None:
            self._cache = dict(qkv=tuple(t.detach() for t in self.decoder.mid_block.attentions[0].qkv()),
                               conv_out=self.padded_conv_out(), post_quant=self.scaled_post_quant_conv())
        return self._cache

    def refresh_derived_(self):
        self._cache = None
        self._gn_ws = {}
        return self

    def _apply(self, fn, recurse=True):          # .to() / .cuda() / .half(): the weights move, the derived ones go
        self.refresh_derived_()
        return super()._apply(fn, recurse)

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.refresh_derived_()
        return out

    def _gn(self, norm, x, silu):
        from mixdq_amd import _C
        N, C, H, W = x.shape
        key = (N, H * W, C, norm.num_groups, x.device)
        ws = self._gn_ws.get(key)
        if ws is None:
            ws = self._gn_ws[key] = _C.groupnorm_workspace(N, H * W, C, norm.num_groups, x.device)
        return _C.groupnorm_silu_quantize(x, norm.num_groups, norm.weight, norm.bias, norm.eps, silu=silu,
                                          want_f16=True, _workspace=ws)[1]

    # ---- forward --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, latents):
        from mixdq_amd import _C
        if not (torch.is_tensor(latents) and latents.is_cuda and latents.dim() == 4
                and latents.shape[1] == self.cfg["latent_channels"]
                and latents.dtype in (torch.float16, torch.float32)):
            raise RuntimeError("VAEDecoder.decode: latents should be a [B, %d, h, w] FP32 or FP16 GPU tensor"
                               % self.cfg["latent_channels"])
        if self.decoder.conv_in.weight.dtype != torch.float16:
            raise RuntimeError("VAEDecoder.decode: the decoder runs in FP16 (build_vae_decoder / .half())")
        d, dec = self._derived(), self.decoder
        z = latents.to(torch.float16).contiguous(memory_format=torch.channels_last)
        x = _C.conv2d_f16(z, *d["post_quant"], 1, 0)
        x = _C.conv2d_f16(x, dec.conv_in.weight, dec.conv_in.bias, 1, 1)        # C = 4: the small-C kernel
        x = dec.mid_block.run(self, x)
        for blk in dec.up_blocks:
            x = blk.run(self, x)
        x = self._gn(dec.conv_norm_out, x, True)
        x = _C.conv2d_f16(x, *d["conv_out"], 1, 1)
        return x[:, :dec.conv_out.out_channels]

    def decode(self, latents):
        """latents [B, 4, h, w] (FP32 or FP16, as a sampler leaves them: still multiplied by scaling_factor) ->
        FP16 [B, 3, 8h, 8w], unclamped, as diffusers' `vae.decode(latents / scaling_factor).sample`."""
        return self.forward(latents)


def to_uint8(image):
    """(image / 2 + 0.5).clamp(0, 1) * 255, rounded: uint8, same shape."""
    return ((image.to(torch.float32) / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8)


def state_dict_names(cfg=None):
    """The parameter names (diffusers') of the decoder half of an AutoencoderKL with this config, written out from
    the layer list rather than read off the modules."""
    cfg = VAE_SDXL_CONFIG if cfg is None else cfg
    ch = tuple(cfg["block_out_channels"])
    rev = ch[::-1]
    names = ["post_quant_conv", "decoder.conv_in"]
    res = lambda p, short: [p + s for s in ("norm1", "conv1", "norm2", "conv2") + (("conv_shortcut",) if short else ())]
    names += ["decoder.mid_block.attentions.0." + s for s in ("group_norm", "to_q", "to_k", "to_v", "to_out.0")]
    for j in range(2):
        names += res(f"decoder.mid_block.resnets.{j}.", False)
    for i in range(len(rev)):
        for j in range(cfg["layers_per_block"] + 1):
            names += res(f"decoder.up_blocks.{i}.resnets.{j}.", j == 0 and rev[max(i - 1, 0)] != rev[i])
        if i != len(rev) - 1:
            names.append(f"decoder.up_blocks.{i}.upsamplers.0.conv")
    names += ["decoder.conv_norm_out", "decoder.conv_out"]
    return [n + sfx for n in names for sfx in (".weight", ".bias")]


def build_vae_decoder(cfg=None, seed: int = 42, device=None, dtype=torch.float16) -> VAEDecoder:
    """A decoder with synthetic weights (randn * 0.02 per conv / linear layer, as build_unet's), FP16, channels-last."""
    from mixdq_amd.unet import init_synthetic_weights
    vae = VAEDecoder(cfg)
    init_synthetic_weights(vae, seed)
    vae = vae.to(dtype=dtype)
    if device is not None:
        vae = vae.to(device)
    vae = vae.to(memory_format=torch.channels_last)
    return vae.eval()


def parameter_counts(vae) -> "OrderedDict[str, int]":
    """Parameters under `decoder.` and under `post_quant_conv.`."""
    out = OrderedDict(decoder=0, post_quant_conv=0)
    for n, p in vae.named_parameters():
        out[n.split(".")[0]] += p.numel()
    return out
