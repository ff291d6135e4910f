"""The FP16 VAE decoder (diffusers' AutoencoderKL.decode) on this library's kernels: latents in, image out.

    vae = build_vae_decoder(VAE_SDXL_CONFIG).cuda()          # synthetic weights; load_state_dict takes diffusers' names
    image = vae.decode(latents)                              # [B, 4, h, w] FP32 / FP16 -> FP16 [B, 3, 8h, 8w]
    pixels = to_uint8(image)

Every layer runs channels-last in FP16 on the C-ABI library: mixdq_conv2d_f16 (the residual of a ResNet block folded
into its second conv, `Upsample2D`'s nearest 2x folded into the conv's gather: MIXDQ_FLAG_UPSAMPLE2X),
mixdq_groupnorm_silu_quantize with its FP16 output, mixdq_linear_f16 (one q|k|v projection, N = 3C) and
mixdq_attention_f16 at head width 512 reading the column slices.  The only torch operators of a decode are the dtype /
layout conversion of the 4-channel input and views; `hip_graph_opt(vae)` captures it.

The other half, image in, latents out (diffusers' AutoencoderKL.encode), is VAEEncoder:

    enc = build_vae_encoder(VAE_SDXL_CONFIG).cuda()
    latents = enc.encode(from_uint8(pixels), noise)          # [B, 3, H, W] uint8 / FP16 / FP32 -> FP32 [B, 4, H/8, W/8]

Its launches are the decoder's, plus three forms of its own: mixdq_image_to_nhwc8_f16 (the ingest: any dtype and
strides -> FP16 NHWC with 8 channels, so that conv_in runs on the MFMA tiles; `encode(image, noise, mask=m)` takes
mixdq_image_to_nhwc8_f16_masked instead, which stores the pixels under the mask as 0.0: the blanked image whose latents
the 9-channel inpainting checkpoints read), mixdq_conv2d_f16 with
MIXDQ_FLAG_PAD_AFTER (`Downsample2D`'s 3x3 / stride 2 conv over F.pad(x, (0, 1, 0, 1)) without the padded tensor) and
mixdq_vae_latent_sample (the posterior sample times scaling_factor).  DESIGN.md section 3.25.

This is a floating-point path with no counterpart in the reference (which reaches the VAE through diffusers'
pipeline): it is held to tolerance against the same network built from stock torch modules (tests/vae_ref.py).
DESIGN.md section 3.23.
"""
import functools
from collections import OrderedDict

import torch
import torch.nn as nn

from mixdq_amd.derived import DerivedWeights

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


def _cat_qkv(_old, wq, bq, wk, bk, wv, bv):
    return torch.cat([wq, wk, wv]).contiguous(), torch.cat([bq, bk, bv]).contiguous()


def _pad_out4(_old, w, b):
    k = w.shape[0]
    k4 = (k + 3) // 4 * 4
    w4 = torch.zeros((k4,) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)
    b4 = torch.zeros(k4, dtype=b.dtype, device=b.device)
    w4[:k], b4[:k] = w.detach(), b.detach()
    return w4.contiguous(memory_format=torch.channels_last), b4


def _scaled(factor, _old, w, b):
    w = w.detach()
    return (w.float() / factor).to(w.dtype).contiguous(memory_format=torch.channels_last), b.detach()


def _pad_in8(_old, w, b):
    from mixdq_amd.nn.Conv2d import pad_in8
    return pad_in8(w.detach()), b.detach()


class VaeAttention(nn.Module):
    """diffusers' Attention as the VAE's mid block uses it: one head as wide as the block, a residual connection."""

    def __init__(self, c, groups):
        super().__init__()
        self.group_norm = nn.GroupNorm(groups, c, eps=GN_EPS)
        self.to_q, self.to_k, self.to_v = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)
        self.to_out = nn.ModuleList([nn.Linear(c, c)])

    def qkv(self):
        """to_q | to_k | to_v as ONE [3C, C] projection."""
        return _cat_qkv(None, *self.qkv_sources())

    def qkv_sources(self):
        return tuple(p for m in (self.to_q, self.to_k, self.to_v) for p in (m.weight, m.bias))

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


class _VaeHalf(DerivedWeights, nn.Module):
    """What the two halves of the AutoencoderKL share: the config, the tensors derived from the weights (the
    subclass's `_derive` declares them; lifecycle: DerivedWeights) and the GroupNorm launch with its cached workspaces,
    which depend on shapes only: a load keeps them, a move or a load that changed the weights' metadata drops them.
    The blocks above reach all three through the `vae` argument of their `run`."""

    def __init__(self, cfg=None):
        super().__init__()
        self.cfg = dict(VAE_SDXL_CONFIG if cfg is None else cfg)
        self.scaling_factor = float(self.cfg["scaling_factor"])
        self._gn_ws = {}           # GroupNorm workspaces, one per (shape, device)
        self._init_derived()

    def _drop_derived(self):
        super()._drop_derived()
        self._gn_ws = {}

    def _gn(self, norm, x, silu):
        from mixdq_amd import _C
        N, C, H, W = x.shape
        key = (N, H * W, C, norm.num_groups, x.device)
        ws = self._gn_ws.get(key)
        if ws is None:
            ws = self._gn_ws[key] = _C.groupnorm_workspace(N, H * W, C, norm.num_groups, x.device)
        return _C.groupnorm_silu_quantize(x, norm.num_groups, norm.weight, norm.bias, norm.eps, silu=silu,
                                          want_f16=True, _workspace=ws)[1]


class VAEDecoder(_VaeHalf):
    """post_quant_conv + decoder of an AutoencoderKL, parameter names as diffusers'."""

    def __init__(self, cfg=None):
        super().__init__(cfg)
        lc = self.cfg["latent_channels"]
        self.post_quant_conv = nn.Conv2d(lc, lc, 1)
        self.decoder = VaeDecoderNet(self.cfg)

    # ---- derived weights ------------------------------------------------------------------------------------
    def padded_conv_out(self):
        """conv_out's weight / bias padded with zero output channels to a multiple of four (3 -> 4), the width the MFMA
        tiles take; decode() returns the first `out_channels` of that conv."""
        return _pad_out4(None, self.decoder.conv_out.weight, self.decoder.conv_out.bias)

    def scaled_post_quant_conv(self):
        """post_quant_conv on z / scaling_factor == the conv with weight / scaling_factor on z (the division is done
        once, in FP32, on the 4 x 4 weight; the bias is untouched)."""
        return _scaled(self.scaling_factor, None, self.post_quant_conv.weight, self.post_quant_conv.bias)

    def _derive(self):
        conv_out, pq = self.decoder.conv_out, self.post_quant_conv
        return dict(qkv=(self.decoder.mid_block.attentions[0].qkv_sources(), _cat_qkv),
                    conv_out=((conv_out.weight, conv_out.bias), _pad_out4),
                    post_quant=((pq.weight, pq.bias), functools.partial(_scaled, self.scaling_factor)))

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


class VaeDownsample(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, stride=2, padding=0)      # over F.pad(x, (0, 1, 0, 1)): padded after, not before


class VaeDownBlock(nn.Module):
    def __init__(self, cin, cout, n_resnets, groups, add_down):
        super().__init__()
        self.resnets = nn.ModuleList([VaeResnetBlock(cin if i == 0 else cout, cout, groups) for i in range(n_resnets)])
        if add_down:
            self.downsamplers = nn.ModuleList([VaeDownsample(cout)])

    def run(self, vae, x):
        from mixdq_amd import _C
        for r in self.resnets:
            x = r.run(vae, x)
        if hasattr(self, "downsamplers"):
            conv = self.downsamplers[0].conv    # the zeros lie below and right only: no padded tensor
            x = _C.conv2d_f16(x, conv.weight, conv.bias, 2, 1, _pad_after=True)
        return x


class VaeEncoderNet(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        ch, g = tuple(cfg["block_out_channels"]), cfg["norm_num_groups"]
        self.conv_in = nn.Conv2d(cfg.get("in_channels", 3), ch[0], 3, padding=1)
        self.down_blocks = nn.ModuleList([
            VaeDownBlock(ch[max(i - 1, 0)], ch[i], cfg["layers_per_block"], g, i != len(ch) - 1)
            for i in range(len(ch))])
        self.mid_block = VaeMidBlock(ch[-1], g)
        self.conv_norm_out = nn.GroupNorm(g, ch[-1], eps=GN_EPS)
        self.conv_out = nn.Conv2d(ch[-1], 2 * cfg["latent_channels"], 3, padding=1)


class VAEEncoder(_VaeHalf):
    """encoder + quant_conv of an AutoencoderKL, parameter names as diffusers'."""

    def __init__(self, cfg=None):
        super().__init__(cfg)
        lc = self.cfg["latent_channels"]
        self.encoder = VaeEncoderNet(self.cfg)
        self.quant_conv = nn.Conv2d(2 * lc, 2 * lc, 1)

    # ---- derived weights ------------------------------------------------------------------------------------
    def padded_conv_in(self):
        """conv_in's weight padded with zero INPUT channels to eight (3 -> 8), the width at which the conv runs on the
        MFMA tiles; the ingest kernel writes the image with eight channels, 3..7 zero."""
        return _pad_in8(None, self.encoder.conv_in.weight, self.encoder.conv_in.bias)

    def _derive(self):
        conv_in = self.encoder.conv_in
        return dict(qkv=(self.encoder.mid_block.attentions[0].qkv_sources(), _cat_qkv),
                    conv_in=((conv_in.weight, conv_in.bias), _pad_in8))

    # ---- forward --------------------------------------------------------------------------------------------
    def _check_image(self, image, what):
        cin = self.encoder.conv_in.in_channels
        if not (torch.is_tensor(image) and image.is_cuda and image.dim() == 4 and image.shape[1] == cin
                and image.dtype in (torch.uint8, torch.float16, torch.float32)
                and image.shape[2] % 8 == 0 and image.shape[3] % 8 == 0):
            raise RuntimeError("VAEEncoder.%s: image should be a [B, %d, H, W] uint8, FP16 or FP32 GPU tensor with H and "
                               "W multiples of 8" % (what, cin))
        if self.encoder.conv_in.weight.dtype != torch.float16:
            raise RuntimeError("VAEEncoder.%s: the encoder runs in FP16 (build_vae_encoder / .half())" % what)

    @torch.no_grad()
    def _moments(self, image, mask=None):
        from mixdq_amd import _C
        d, enc = self._derived(), self.encoder
        x = _C.image_to_nhwc8_f16(image, mask)                            # any dtype and strides -> FP16, 8 channels
        x = _C.conv2d_f16(x, *d["conv_in"], 1, 1)
        for blk in enc.down_blocks:
            x = blk.run(self, x)
        x = enc.mid_block.run(self, x)
        x = self._gn(enc.conv_norm_out, x, True)
        x = _C.conv2d_f16(x, enc.conv_out.weight, enc.conv_out.bias, 1, 1)
        return _C.conv2d_f16(x, self.quant_conv.weight, self.quant_conv.bias, 1, 0)

    def moments(self, image):
        """image -> FP16 [B, 2L, H/8, W/8] channels-last: the posterior's mean (channels 0..L-1) and log-variance, as
        diffusers' `vae.quant_conv(vae.encoder(image))`."""
        self._check_image(image, "moments")
        return self._moments(image)

    @torch.no_grad()
    def forward(self, image, noise=None, mask=None):
        from mixdq_amd import _C
        self._check_image(image, "encode")
        if mask is not None and not (torch.is_tensor(mask) and mask.device == image.device
                                     and mask.dtype in (torch.uint8, torch.float16, torch.float32)
                                     and tuple(mask.shape) in ((image.shape[0],) + tuple(image.shape[2:]),
                                                               (image.shape[0], 1) + tuple(image.shape[2:]))):
            raise RuntimeError("VAEEncoder.encode: mask should be a [B, H, W] or [B, 1, H, W] uint8, FP16 or FP32 "
                               "tensor of the image's size on its device")
        if noise is not None:
            want = (image.shape[0], self.cfg["latent_channels"], image.shape[2] // 8, image.shape[3] // 8)
            if not (torch.is_tensor(noise) and noise.device == image.device and noise.dtype == torch.float32
                    and tuple(noise.shape) == want):
                raise RuntimeError("VAEEncoder.encode: noise should be an FP32 tensor of shape %s on the image's device"
                                   % (want,))
            noise = noise.contiguous(memory_format=torch.channels_last)
        return _C.vae_latent_sample(self._moments(image, mask), noise, self.scaling_factor)

    def encode(self, image, noise=None, mask=None):
        """image [B, 3, H, W] (uint8: a pixel u is u / 127.5 - 1; FP16 / FP32: already in [-1, 1]; any strides; H and
        W multiples of 8) -> FP32 [B, L, H/8, W/8] channels-last, already multiplied by scaling_factor: with `noise`
        (FP32, the result's shape) diffusers' `vae.encode(x).latent_dist.sample() * scaling_factor`, without it
        `.mode() * scaling_factor`.  What Sampler.sample(init_latents=...) takes.

        `mask` ([B, H, W] or [B, 1, H, W] at the image's size; uint8 >= 128 or float >= 0.5 is set; any strides): the
        pixels under it enter the encoder as 0.0 -- mid-grey -- in every channel (mixdq_image_to_nhwc8_f16_masked in
        place of the plain ingest, nothing else differs): diffusers' `init_image * (mask < 0.5)`, the masked image whose
        latents a 9-channel inpainting UNet is conditioned on (_C.inpaint_cond)."""
        if mask is None:
            return self.forward(image, noise)
        return self.forward(image, noise, mask)


def to_uint8(image):
    """(image / 2 + 0.5).clamp(0, 1) * 255, rounded: uint8, same shape."""
    return ((image.to(torch.float32) / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8)


def composite_uint8(decoded, original, mask):
    """Inpainting's last step, one launch (mixdq_composite_u8): to_uint8(decoded) where `mask` (image resolution,
    [B, H, W] or [B, 1, H, W]; uint8 >= 128 or float >= 0.5 is set) is set, `original`'s bytes elsewhere -- every pixel
    outside the mask comes back bit-identical, which the VAE round trip alone does not give.  decoded: FP16
    [B, 3, H, W] as VAEDecoder.decode returns it; original: uint8, same shape, any strides.  uint8, channels-last."""
    from mixdq_amd import _C
    return _C.composite_u8(decoded, original, mask)


def from_uint8(pixels):
    """The inverse of to_uint8: uint8 -> FP16 in [-1, 1], f16(f32(u) * f32(2 / 255) - 1) with each FP32 operation
    rounded -- the ingest kernel's uint8 arithmetic (mixdq_image_to_nhwc8_f16) restated in torch.  For every u it is
    f16(u / 127.5 - 1), diffusers' (u / 255) * 2 - 1 in FP32 rounded to FP16, and to_uint8 of it is u."""
    return (pixels.to(torch.float32) * torch.tensor(2.0 / 255.0, dtype=torch.float32) - 1.0).to(torch.float16)


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


def encoder_state_dict_names(cfg=None):
    """The parameter names (diffusers') of the encoder half of an AutoencoderKL with this config, written out from
    the layer list rather than read off the modules."""
    cfg = VAE_SDXL_CONFIG if cfg is None else cfg
    ch = tuple(cfg["block_out_channels"])
    names = ["quant_conv", "encoder.conv_in"]
    res = lambda p, short: [p + s for s in ("norm1", "conv1", "norm2", "conv2") + (("conv_shortcut",) if short else ())]
    for i in range(len(ch)):
        for j in range(cfg["layers_per_block"]):
            names += res(f"encoder.down_blocks.{i}.resnets.{j}.", j == 0 and ch[max(i - 1, 0)] != ch[i])
        if i != len(ch) - 1:
            names.append(f"encoder.down_blocks.{i}.downsamplers.0.conv")
    names += ["encoder.mid_block.attentions.0." + s for s in ("group_norm", "to_q", "to_k", "to_v", "to_out.0")]
    for j in range(2):
        names += res(f"encoder.mid_block.resnets.{j}.", False)
    names += ["encoder.conv_norm_out", "encoder.conv_out"]
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


def build_vae_encoder(cfg=None, seed: int = 42, device=None, dtype=torch.float16) -> VAEEncoder:
    """An encoder with synthetic weights (as build_vae_decoder's), FP16, channels-last."""
    from mixdq_amd.unet import init_synthetic_weights
    vae = VAEEncoder(cfg)
    init_synthetic_weights(vae, seed)
    vae = vae.to(dtype=dtype)
    if device is not None:
        vae = vae.to(device)
    vae = vae.to(memory_format=torch.channels_last)
    return vae.eval()


def parameter_counts(vae) -> "OrderedDict[str, int]":
    """Parameters by top-level module: `decoder` and `post_quant_conv` (a VAEDecoder), `encoder` and `quant_conv` (a
    VAEEncoder)."""
    out = OrderedDict((k, 0) for k in (("encoder", "quant_conv") if isinstance(vae, VAEEncoder) else
                                       ("decoder", "post_quant_conv")))
    for n, p in vae.named_parameters():
        out[n.split(".")[0]] += p.numel()
    return out
