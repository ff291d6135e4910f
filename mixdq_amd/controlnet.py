"""diffusers' ControlNetModel on this repository's blocks, with its parameter names.

A ControlNet is the UNet's encoder half -- conv_in, time_embedding, [add_embedding], down_blocks, mid_block: the classes
of mixdq_amd/unet.py, so calibrate / quantize_unet / set_fused(True) treat it like a UNet -- plus

    controlnet_cond_embedding   eight small 3x3 convs that take the hint image [B, 3, 8h, 8w] in [0, 1] down to the
                                latent grid: conv_in, blocks.0..5 (stride 1 and stride 2 alternating), conv_out
    controlnet_down_blocks.i    one 1x1 conv per skip tensor (conv_in's output first): the "zero convs"
    controlnet_mid_block        one 1x1 conv on the mid-block output

forward() returns the residuals UNSCALED: SDXLUNet.forward(control=ControlResiduals(...)) scales and adds them in one
launch (mixdq_control_add_f16), with scales read from a device table at the device-side step, so that one captured
graph serves every conditioning scale and guidance window.

The hint does not change during a run, so what the conditioning embedding makes of it is computed once per call
(hint_term(), outside a captured graph: the idea of SDXLUNet.cond_term) and enters every step as the residual of
conv_in's epilogue.  These layers stay FP16: conv_in, the conditioning embedding and the 1x1 convs are to be left out of
the activation bit-width config; a quantized conv_in is refused.

Not here: guess_mode, ControlNet-XS, a quantized hint embedding.  Skipping the ControlNet's forward itself while its
guidance window is closed: a captured graph cannot branch, so only its residuals' loads are saved then.
Weights are synthetic (init_synthetic_weights: the "zero convs" are NOT zero there)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from mixdq_amd import derived
from mixdq_amd import unet as U
from mixdq_amd.unet import (DownBlock, FusedGraph, MidBlock, SD15_CONFIG, SD21_CONFIG, SDXL_CONFIG, TimestepEmbedding,
                            init_synthetic_weights)

_HINT = dict(conditioning_embedding_out_channels=(16, 32, 96, 256), conditioning_channels=3)
CONTROLNET_SD15_CONFIG = dict(SD15_CONFIG, **_HINT)          # 361 279 120 parameters (the published figure)
CONTROLNET_SDXL_CONFIG = dict(SDXL_CONFIG, **_HINT)          # 1 251 014 160
CONTROLNET_SD21_CONFIG = dict(SD21_CONFIG, **_HINT)          # 364 228 240

MAX_NETS = 4


class ControlNetConditioningEmbedding(nn.Module):
    """conv_in (3x3) -> SiLU -> [blocks.2i: 3x3 stride 1 -> SiLU -> blocks.2i+1: 3x3 stride 2 -> SiLU] -> conv_out (3x3),
    every conv with padding 1: three halvings, image to latent grid."""

    def __init__(self, out_channels, channels=(16, 32, 96, 256), in_channels=3):
        super().__init__()
        self.conv_in = nn.Conv2d(in_channels, channels[0], 3, 1, 1)
        self.blocks = nn.ModuleList()
        for a, b in zip(channels[:-1], channels[1:]):
            self.blocks.append(nn.Conv2d(a, a, 3, 1, 1))
            self.blocks.append(nn.Conv2d(a, b, 3, 2, 1))
        self.conv_out = nn.Conv2d(channels[-1], out_channels, 3, 1, 1)

    def forward(self, x):                         # the stock form: calibration, the CPU, other dtypes
        x = F.silu(self.conv_in(x))
        for blk in self.blocks:
            x = F.silu(blk(x))
        return self.conv_out(x)


def _hooked(layer) -> bool:
    """Someone watches this layer's calls (calibrate's forward pre-hooks): it then runs as the module it is."""
    return bool(layer._forward_pre_hooks or layer._forward_hooks)


def _fp16_conv(layer, x, residual=None):
    """An FP16 conv layer (nn.Conv2d, or the FP fallback of a converted one) on this library's FP16 conv launch;
    elsewhere (CPU, other dtypes, a watched layer) the module itself."""
    w = getattr(layer, "weight", None)
    if (w is None or getattr(layer, "valid_for_acceleration", False) or _hooked(layer)
            or not (x.is_cuda and x.dtype == torch.float16 and w.dtype == torch.float16)):
        y = layer(x)
        return y if residual is None else y + residual
    from mixdq_amd import _C
    y = _C.conv2d_f16(x, w, layer.bias, layer.stride[0], layer.padding[0],
                      _residual=None if U.DEFUSE else residual)
    return y + residual if (U.DEFUSE and residual is not None) else y


class ControlNet(FusedGraph):
    """forward(sample, timestep, encoder_hidden_states, added_cond_kwargs=None, *, hint_term) -> (down residuals, mid
    residual), unscaled; or diffusers' call shape forward(..., controlnet_cond=image, conditioning_scale=1.0), which
    computes the term itself and multiplies in torch.  `cfg`: a UNet config plus conditioning_embedding_out_channels."""

    def __init__(self, cfg=None):
        super().__init__()
        cfg = dict(CONTROLNET_SDXL_CONFIG, **(cfg or {}))
        if cfg["in_channels"] != cfg["out_channels"]:
            raise ValueError("ControlNet: a ControlNet reads the latent channels only (in_channels == out_channels)")
        self.cfg = cfg
        boc = cfg["block_out_channels"]
        temb = cfg["time_embed_dim"]
        self.conv_in = nn.Conv2d(cfg["in_channels"], boc[0], 3, 1, 1)
        self.time_embedding = TimestepEmbedding(boc[0], temb)
        if cfg.get("addition_embed_type", "text_time") is not None:
            self.add_embedding = TimestepEmbedding(cfg["projection_class_embeddings_input_dim"], temb)
        self.controlnet_cond_embedding = ControlNetConditioningEmbedding(
            boc[0], tuple(cfg["conditioning_embedding_out_channels"]), cfg.get("conditioning_channels", 3))
        n = cfg["layers_per_block"]
        depths = cfg["transformer_layers_per_block"]
        self.down_blocks = nn.ModuleList()
        self.controlnet_down_blocks = nn.ModuleList([nn.Conv2d(boc[0], boc[0], 1)])
        cin = boc[0]
        for i, cout in enumerate(boc):
            last = i == len(boc) - 1
            self.down_blocks.append(DownBlock(cin, cout, temb, n, depths[i], cfg, not last))
            for _ in range(n + (0 if last else 1)):
                self.controlnet_down_blocks.append(nn.Conv2d(cout, cout, 1))
            cin = cout
        self.mid_block = MidBlock(boc[-1], temb, cfg["mid_transformer_layers"], cfg)
        self.controlnet_mid_block = nn.Conv2d(boc[-1], boc[-1], 1)
        self.register_load_state_dict_post_hook(derived.after_load)

    # ---- the hint ----------------------------------------------------------------------------------------------
    def _fp16_conv_in(self):
        if getattr(self.conv_in, "valid_for_acceleration", False) or getattr(self.conv_in, "weight", None) is None:
            raise RuntimeError("ControlNet: conv_in takes the hint term as the residual of its epilogue and needs to be a "
                               "floating-point layer: leave 'conv_in' out of the activation bit-width config")
        return self.conv_in

    def _check_image(self, image, what):
        c = self.cfg.get("conditioning_channels", 3)
        if not (torch.is_tensor(image) and image.dim() == 4 and image.shape[1] == c
                and image.dtype in (torch.uint8, torch.float16, torch.float32)
                and image.shape[2] % 8 == 0 and image.shape[3] % 8 == 0 and image.shape[2] > 0 and image.shape[3] > 0):
            raise RuntimeError(f"ControlNet.{what}: the hint image should be a uint8, fp16 or fp32 [B, {c}, 8h, 8w] tensor "
                               "with values in [0, 1] (uint8: 0..255)")

    @torch.no_grad()
    def hint_term(self, image):
        """What the conditioning embedding makes of the hint image: image [B, 3, 8h, 8w], uint8 (0..255), fp16 or fp32
        (in [0, 1]; no clamp) of any strides -> fp16 channels-last [B, C0, h, w].  On the GPU: the ingest
        (_C.hint_to_nhwc8_f16: uint8 u becomes f16(u / 255)), seven FP16 convs each followed by an in-place SiLU launch,
        and conv_out -- this library's launches all.  Runs once per call, outside a captured graph; pass the result as
        forward(..., hint_term=T) at every step (one row per sample row).  The 8-channel forms of the two convs with
        fewer input channels -- this embedding's conv_in and the trunk's conv_in -- are re-derived here, in place,
        when their weights were replaced or written since."""
        self._check_image(image, "hint_term")
        emb = self.controlnet_cond_embedding
        layers = [emb.conv_in] + list(emb.blocks) + [emb.conv_out]
        w0 = getattr(emb.conv_in, "weight", None)
        stock = (w0 is None or not image.is_cuda or w0.dtype != torch.float16 or w0.device != image.device
                 or any(getattr(l, "valid_for_acceleration", False) or _hooked(l) for l in layers))
        self._fp16_conv_in()
        if image.is_cuda and image.device == self.conv_in.weight.device:
            self._conv_in_split(refresh=True)             # (the trunk's conv_in, padded to 8 channels: read by forward)
        if stock:
            if w0 is not None and image.device != w0.device:
                raise RuntimeError(f"ControlNet.hint_term: the hint image should be on {w0.device}")
            dtype = w0.dtype if w0 is not None else torch.float16
            x = image.float().div(255).to(dtype) if image.dtype == torch.uint8 else image.to(dtype)
            return emb(x).contiguous(memory_format=torch.channels_last)
        from mixdq_amd import _C
        from mixdq_amd.nn.Conv2d import _padded_weight
        (w8,) = derived.derive(derived.holder_of(self), "hint_in8", (w0,), _padded_weight)
        x = _C.hint_to_nhwc8_f16(image)
        y = _C.conv2d_f16(x, w8, emb.conv_in.bias, 1, 1)
        x = _C.silu_f16(y, out=y)
        for blk in emb.blocks:
            y = _C.conv2d_f16(x, blk.weight, blk.bias, blk.stride[0], 1)
            x = _C.silu_f16(y, out=y)
        return _C.conv2d_f16(x, emb.conv_out.weight, emb.conv_out.bias, 1, 1)

    def _check_hint_term(self, sample, term):
        want = (sample.shape[0], self.conv_in.out_channels, sample.shape[2], sample.shape[3])
        if not (torch.is_tensor(term) and tuple(term.shape) == want and term.dtype == sample.dtype
                and term.device == sample.device and term.is_contiguous(memory_format=torch.channels_last)):
            raise RuntimeError(f"ControlNet.forward: hint_term should be a channels-last {sample.dtype} tensor of shape "
                               f"{want} (one row per sample row) on the sample's device")

    def _conv_in_hint(self, x, term):
        """conv_in of a step plus the hint: f16(f32(f16(conv + bias)) + f32(T)), diffusers' conv_in(sample) + cond as
        the residual of the conv's epilogue (the 4-channel conv padded to 8 channels)."""
        conv = self._fp16_conv_in()
        if _hooked(conv) or not (x.is_cuda and x.dtype == torch.float16 and conv.weight.dtype == torch.float16):
            return conv(x) + term
        wx, _ = self._conv_in_split(refresh=False)
        from mixdq_amd import _C
        x8 = self._pad8(x)
        if U.DEFUSE:
            return _C.conv2d_f16(x8, wx, conv.bias, 1, 1) + term
        return _C.conv2d_f16(x8, wx, conv.bias, 1, 1, _residual=term)

    def _conv_in_split(self, refresh: bool):
        if not refresh and derived.stored(self.__dict__.get("_derived_tensors"), "cin_split") is None:
            raise RuntimeError("ControlNet.forward: hint_term= should be what this ControlNet's hint_term() returned")
        return super()._conv_in_split(refresh)

    # ---- the step ----------------------------------------------------------------------------------------------
    def n_skips(self) -> int:
        return len(self.controlnet_down_blocks)

    def forward(self, sample, timestep, encoder_hidden_states, added_cond_kwargs=None, *, hint_term=None,
                controlnet_cond=None, conditioning_scale=1.0, return_dict=False):
        if sample.dim() != 4 or sample.shape[1] != self.cfg["in_channels"]:
            raise RuntimeError(f"ControlNet.forward: sample should be [B, {self.cfg['in_channels']}, h, w]")
        if (hint_term is None) == (controlnet_cond is None):
            raise RuntimeError("ControlNet.forward: pass hint_term= (what hint_term(image) returned) or controlnet_cond= "
                               "(the hint image), one of the two")
        dropin = hint_term is None
        if dropin:
            self._check_image(controlnet_cond, "forward")
            if controlnet_cond.shape[0] != sample.shape[0] or tuple(controlnet_cond.shape[2:]) != (
                    8 * sample.shape[2], 8 * sample.shape[3]):
                raise RuntimeError("ControlNet.forward: controlnet_cond should have the sample's batch and 8 times its "
                                   "height and width")
            hint_term = self.hint_term(controlnet_cond).to(sample.dtype)
        self._check_hint_term(sample, hint_term)
        emb = self._embed(sample, timestep, added_cond_kwargs)
        down, mid = self._with_prefetch(sample, lambda: self._forward_body(sample, emb, encoder_hidden_states, hint_term))
        if dropin and conditioning_scale != 1.0:
            down, mid = [d * conditioning_scale for d in down], mid * conditioning_scale
        return down, mid

    def _forward_body(self, sample, emb, encoder_hidden_states, hint_term):
        if self.fused and U._fusable_f16(sample) and not U.DEFUSE:
            self._project_temb_ahead(emb)
            self._project_context_ahead(encoder_hidden_states)
        x = sample.contiguous(memory_format=torch.channels_last)
        x = self._conv_in_hint(x, hint_term)
        skips = [x]
        for blk in self.down_blocks:
            x, outs = blk(x, emb, encoder_hidden_states)
            skips += outs
        x = self.mid_block(x, emb, encoder_hidden_states)
        cl = torch.channels_last                          # (what SDXLUNet.forward asks of a residual; no copy on the GPU)
        down = [_fp16_conv(conv, s).contiguous(memory_format=cl) for conv, s in zip(self.controlnet_down_blocks, skips)]
        return down, _fp16_conv(self.controlnet_mid_block, x).contiguous(memory_format=cl)


def build_controlnet(device=None, dtype=torch.float16, seed: int = 4242, cfg=None) -> ControlNet:
    """A ControlNet with synthetic weights (init_synthetic_weights: every layer randn * 0.02, the zero convs too)."""
    net = ControlNet(cfg)
    init_synthetic_weights(net, seed)
    net = net.to(dtype=dtype)
    if device is not None:
        net = net.to(device)
    net = net.to(memory_format=torch.channels_last)
    return net.eval()


def control_scale_table(n_steps, t0, scales, starts, ends):
    """The fp32 [K, n_steps] table of conditioning scales of a run (numpy): the run takes the m = n_steps - t0 steps
    t0 .. n_steps - 1 (t0 > 0: an img2img start), and at its step j net k is on unless j / m < start_k or
    (j + 1) / m > end_k -- diffusers' control_guidance_start / control_guidance_end rule, in Python floats:
    table[k, t0 + j] = f32(scale_k * keep), every other entry 0 (a net whose entry is 0 is skipped by control_add)."""
    K = len(scales)
    if not (len(starts) == K and len(ends) == K):
        raise ValueError("control_scale_table: one scale, start and end per net")
    if not 0 <= t0 < n_steps:
        raise ValueError(f"control_scale_table: the first step {t0} should lie in [0, {n_steps})")
    m = n_steps - t0
    table = np.zeros((K, n_steps), np.float32)
    for k in range(K):
        s, e = float(starts[k]), float(ends[k])
        if not (0.0 <= s <= 1.0 and 0.0 <= e <= 1.0 and s <= e):
            raise ValueError(f"control_scale_table: net {k}: 0 <= control_start <= control_end <= 1, got ({s}, {e})")
        for j in range(m):
            keep = 1.0 - float(j / m < s or (j + 1) / m > e)
            table[k, t0 + j] = np.float32(float(scales[k]) * keep)
    return table
