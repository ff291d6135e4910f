"""SDXL(-Turbo) UNet graph with diffusers-compatible module names.

diffusers is not installed anywhere this repo runs, and the reference's harness
(kernels/quantize_sdxl.py:331-484) drives `pipeline.unet`.  This module is a structural clone of
`UNet2DConditionModel` for the SDXL config (block channels 320/640/1280, transformer depth
0/2/10 + mid 10, cross-attention dim 2048, text_time addition embedding 2816 -> 1280) whose
`named_modules()` reproduce exactly the 794 quantizable layer names of the reference's bit-width
yamls (743 Linear + 51 Conv2d), so `quantize_unet` drops in unchanged.
Every Linear/Conv2d is a plain nn.Linear/nn.Conv2d until `mixdq_amd.quantize.convert` swaps it.

The glue between quantized layers (GroupNorm, SiLU, LayerNorm, GEGLU, scaled-dot-product
attention, nearest upsample) stays FP16 PyTorch, as in the reference (SURVEY.md section 0:
the reference fuses none of it and runs attention in FP16).  Activations are kept channels-last
so the INT8 NHWC conv never converts layouts (qconv2d.cc:91-95 would copy).

Weights are synthetic (no network, no checkpoints): randn * 0.02, seeded per layer.
"""
from __future__ import annotations

import functools
import math
import os
import weakref
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from mixdq_amd import derived

# ---------------------------------------------------------------------------------------------
# Fused forward.  With `unet.fused = True` (set_fused) the glue that
# feeds a W8A8 layer is replaced by the producer-fusion kernels of mixdq_amd/csrc/fused_norm.hip
# and the residual adds move into the GEMM / conv epilogues.  Rounding points are those of the
# unfused graph; the only numerical difference is this repo's GroupNorm / LayerNorm / SiLU / GELU
# arithmetic (include/mixdq_math.h, fixed reduction order) instead of PyTorch's, i.e. at most
# one FP16 ulp before quantization.  Off by default: the unfused graph is the drop-in path.
# ---------------------------------------------------------------------------------------------
# De-fused reference of the fused graph (tests/test_unet_full_gpu.py): with DEFUSE on, the fused
# forward keeps its structure but every fused launch is replaced by the chain of THIS repo's
# kernels it stands for -- GroupNorm / LayerNorm / GEGLU / attention with FP16 output followed by
# the layer's own quantize launch, separate to_q / to_k / to_v and K / V GEMMs, torch half adds in
# place of the residual epilogues, torch.cat in place of the two-source reads.  Same arithmetic at
# every rounding point, so the two graphs agree BIT FOR BIT and any difference is a wiring mistake.
DEFUSE = False


class defused:
    """`with defused(): unet(...)` runs the de-fused reference of the fused graph."""

    def __enter__(self):
        global DEFUSE
        self.saved, DEFUSE = DEFUSE, True

    def __exit__(self, *exc):
        global DEFUSE
        DEFUSE = self.saved


# MIXDQ_CONTROL_ADD=0: the fused forward adds ControlNet residuals with torch half operations instead of the
# control_add launch (A/B runs and tests; read once per process).  The torch form reads the scales of the step on the
# host, so it cannot be captured into a graph.
CONTROL_ADD = not os.environ.get("MIXDQ_CONTROL_ADD", "1").startswith("0")


class ControlResiduals:
    """What SDXLUNet.forward(control=...) adds to its skip tensors and to the mid-block output.

    nets:   per ControlNet (1 to 4) the pair (down residuals, mid residual) as ControlNet.forward returns it, UNSCALED:
            one tensor per skip of the UNet (conv_in's output first) and one for the mid-block output
    scales: fp32 [K, n_steps] on the residuals' device: scales[k, j] is net k's conditioning scale at step j (0 while its
            guidance window is closed: the net is then skipped)
    step:   one int32 on that device, the step counter (the one the sampler step advances)

    skip_i + (f16(r_0i * c_0) + f16(r_1i * c_1) + ...) in fp16, left to right -- diffusers' arithmetic; include/mixdq_math.h,
    mixdq_control_*."""

    def __init__(self, nets, scales, step):
        self.nets = [(list(down), mid) for down, mid in nets]
        self.scales = scales
        self.step = step


def _accel(m) -> bool:
    if DEFUSE:
        return False
    return bool(getattr(m, "valid_for_acceleration", False)) and not getattr(m, "bos", False) \
        and getattr(m, "split", 0) == 0


def _qp(m):
    return (m.act_scales_inv, m.act_zero_points)


def _abits(m) -> int:
    """Width of a layer's activation quantizer: 8, or 4 for an a4_kernel layer (QuantizedLinear.act_bits).  A
    producer that writes the layer's INT8 operand must clamp to it (include/mixdq_hip.h MIXDQ_FLAG_A4_0)."""
    return getattr(m, "act_bits", 8)


def _a8(m) -> bool:
    """The layer's quantizer is an 8-bit one: the producers that refuse a 4-bit clamp (GroupNorm, GEMM + GEGLU,
    GEMM + LayerNorm) may write its operand."""
    return _abits(m) == 8


def _same_qparams(a, b) -> bool:
    """Host comparison of two layers' activation quantizers -- qparams AND width (a device sync: cached by
    callers, and only ever evaluated in the eager warm-up that precedes graph capture)."""
    return bool(torch.equal(a.act_scales_inv, b.act_scales_inv)
                and torch.equal(a.act_zero_points, b.act_zero_points) and _abits(a) == _abits(b))


def _fusable_f16(x) -> bool:
    return x.is_cuda and x.dtype == torch.float16


# (What is cached on the modules and when it is stale: DESIGN.md "Derived tensors".)
def _quantizer_groups(holder: dict, key, layers):
    """Group id per layer: equal activation quantizers -- qparams and width (8 / 4 bits) -- <=> equal id.  One
    device->host copy (a sync: only ever taken in the eager warm-up that precedes graph capture), memoised in
    `holder[key]` with the derived tensors' freshness test: the qparam tensors, their versions, the widths."""
    src = [t for m in layers for t in (m.act_scales_inv, m.act_zero_points)]
    bits = tuple(_abits(m) for m in layers)
    e = holder.get(key)
    if derived.fresh(e, src, bits):
        return e[2]
    ids = []
    if layers:
        vals = torch.stack([t.detach().reshape(-1)[0].float() for t in src]).cpu().tolist()
        seen = {}
        for i in range(len(layers)):
            ids.append(seen.setdefault((vals[2 * i], vals[2 * i + 1], bits[i]), len(seen)))
    holder[key] = derived.record(src, bits, ids)
    return ids


def _split_pad8(co, _old, w):
    """Builder of the split conv_in weights: w[:, :co] and w[:, co:], each padded to 8 input channels."""
    from mixdq_amd.nn.Conv2d import pad_in8
    return pad_in8(w[:, :co]), pad_in8(w[:, co:])


def _memo(mod) -> dict:
    return mod.__dict__.setdefault("_mixdq_memo", {})


_PACK_VECS = (("wscale", "weight_scales"), ("wsum", "weight_sum_by_input_channels"),
              ("scale", "scale"), ("bias0", "bias0"))


def _wbits(m) -> int:
    """Bits per stored weight value of a quantized Linear: 8 (int8), 4 (packed W4) or 2 (packed W2)."""
    return 2 if getattr(m, "w_packed2", False) else 4 if m.w_packed4 else 8


_WBUF = {8: "weight_int", 4: "weight_int4", 2: "weight_int2"}


def _uniform_storage(layers) -> bool:
    """Layers that are to share one GEMM must store their weights alike (all int8, all packed
    4-bit or all packed 2-bit).  A pure check: the forward never changes a module's buffers -- mixed
    groups are unified once, by `unify_packed_storage_` from `SDXLUNet.set_fused`, or run unpacked."""
    return len({_wbits(m) for m in layers}) == 1


def unify_packed_storage_(layers) -> bool:
    """Explicit post-conversion step (SDXLUNet.set_fused -> prepare_fused_): in a mixed-precision
    config to_q / to_k / to_v (or to_k / to_v) may mix int8, packed 4-bit and packed 2-bit layers.
    With an int8 member every packed one is widened to int8 STORAGE; a mix of 2- and 4-bit only widens
    the 2-bit members to W4 (the values stay the layers' own integers, so every output is unchanged) --
    one launch instead of three is worth more than those layers' smaller bytes.  Replaces the
    `weight_int4` / `weight_int2` buffer by the wider one: state-dict keys change HERE, once, on every
    rank alike, never inside a forward.  Returns whether the group is uniform afterwards."""
    if _uniform_storage(layers):
        return True
    if any(getattr(m, _WBUF[_wbits(m)], None) is None for m in layers):
        return False
    from mixdq_amd.nn.utils import pack_w4
    target = min(8, max(_wbits(m) for m in layers))
    with torch.no_grad():
        for m in layers:
            bits = _wbits(m)
            if bits == target:
                continue
            w = m._weight_values().contiguous()
            delattr(m, _WBUF[bits])
            m.register_buffer(_WBUF[target], w if target == 8 else pack_w4(w))
            m.w_packed2 = False
            m.w_packed4 = target == 4
    return True


def _pack_rows(layers):
    """Row-concatenate the weights and per-channel epilogue vectors of Linear layers that read the
    same INT8 operand: one GEMM against [sum N_i, K] computes every output element exactly as the
    separate launches do.  The concatenated tensors are the storage; the layers keep views."""
    wbits = _wbits(layers[0])
    names = (("w", _WBUF[wbits]),) + _PACK_VECS
    pack = dict(w4=wbits == 4, w2=wbits == 2, wbits=wbits, C=layers[0].out_features, layers=tuple(weakref.ref(m) for m in layers),
                names=names)
    with torch.no_grad():
        for key, name in names:
            cat = torch.cat([getattr(m, name) for m in layers], dim=0).contiguous()
            off = 0
            for m in layers:
                n = getattr(m, name).shape[0]
                setattr(m, name, cat[off:off + n])        # registered buffer -> view of the pack
                off += n
            pack[key] = cat
    return pack


def _pack_valid(pack, layers) -> bool:
    """The layers' buffers still alias the pack (false after a module swap, `.to()`, deepcopy...)."""
    if pack is None or len(pack["layers"]) != len(layers) or any(
            a() is not b for a, b in zip(pack["layers"], layers)):
        return False
    for key, name in pack["names"]:
        cat, off = pack[key], 0
        row = cat.stride(0) * cat.element_size()
        for m in layers:
            t = getattr(m, name, None)
            if (not torch.is_tensor(t) or t.device != cat.device
                    or t.data_ptr() != cat.data_ptr() + off * row):
                return False
            off += t.shape[0]
    return True


def _gn_feed(norm: nn.GroupNorm, x, consumer, silu: bool, x2=None, raw_for=None):
    """GroupNorm(+SiLU) of a channels-last fp16 x for `consumer`: returns (tensor, quantized?).
    x2: the norm is over cat([x, x2], dim=1), read from the two tensors in place.
    raw_for: a W8A8 conv that reads the norm's INPUT (the ResNet 1x1 shortcut, split when x2 is
    given); the return value gains a third element: the input(s) quantized for it by the same pass
    (a list, one INT8 tensor per source), or None when that pass is not the HIP kernel."""
    from mixdq_amd import _C
    if DEFUSE and x2 is not None:
        x, x2 = torch.cat([x, x2], dim=1), None
    N, C, H, W = x.shape
    C += 0 if x2 is None else x2.shape[1]
    if (_fusable_f16(x) and x.is_contiguous(memory_format=torch.channels_last)
            and (x2 is None or (_fusable_f16(x2)
                                and x2.is_contiguous(memory_format=torch.channels_last)
                                and x.shape[1] % 8 == 0 and x2.shape[1] % 8 == 0))
            and _C.groupnorm_supported(N, H * W, C, norm.num_groups)):
        raw_qp = None
        if (GN_RAW_OUTPUTS and not DEFUSE and raw_for is not None
                and getattr(raw_for, "valid_for_acceleration", False)
                and not getattr(raw_for, "bos", False)
                and raw_for.split == (0 if x2 is None else x.shape[1])):
            raw_qp = [(raw_for.act_scales_inv, raw_for.act_zero_points)]
            if x2 is not None:
                raw_qp.append((raw_for.act_scales_inv_0, raw_for.act_zero_points_0))
        if _accel(consumer) and _a8(consumer):      # (the GroupNorm launch writes 8-bit operands only)
            out = _C.groupnorm_silu_quantize(x, norm.num_groups, norm.weight, norm.bias, norm.eps,
                                             *_qp(consumer), silu=silu, x2=x2, raw_qparams=raw_qp)
            res = (out[0], True)
        else:
            out = _C.groupnorm_silu_quantize(x, norm.num_groups, norm.weight, norm.bias, norm.eps,
                                             silu=silu, want_f16=True, x2=x2, raw_qparams=raw_qp)
            res = (out[1], False)
        if raw_for is None:
            return res
        return res + (out[2] if raw_qp is not None else None,)
    if x2 is not None:
        x = torch.cat([x, x2], dim=1)
    # (the stock op by FUNCTION: a module swapped by swap_glue may fold the SiLU into its own launch)
    h = F.group_norm(x, norm.num_groups, norm.weight, norm.bias, norm.eps)
    res = ((F.silu(h) if silu else h), False)
    return res if raw_for is None else res + (None,)


_SHORTCUT_STREAMS = {}
# ResNet 1x1 shortcut convs beside norm1 / conv1 / norm2 on a side stream?  Off: measured on
# MI355X / ROCm 7.2, every extra branch in the captured hipGraph costs more than the kernels it
# overlaps (shortcut branch: 14.40 -> 13.70 ms per step without it; the K/V + time-embedding
# branch: -0.5 ms) -- the step is one chain of launches on one stream.  MIXDQ_SHORTCUT_STREAM=1
# restores the branch for A/B runs.
SHORTCUT_SIDE_STREAM = __import__("os").environ.get("MIXDQ_SHORTCUT_STREAM", "0") == "1"
# norm1's apply pass also writes the shortcut conv's INT8 operand(s) (MIXDQ_GN_RAW=0: separate
# quantize launches, for A/B runs)
GN_RAW_OUTPUTS = __import__("os").environ.get("MIXDQ_GN_RAW", "1") == "1"


def _shortcut_stream(device):
    s = _SHORTCUT_STREAMS.get(device)
    if s is None:
        s = _SHORTCUT_STREAMS[device] = torch.cuda.Stream(device=device)
    return s


def _ln_feed(norm: nn.LayerNorm, x, consumers):
    """LayerNorm of x [B, T, C] for several consumer layers: one fused kernel produces an int8
    tensor per distinct activation quantizer (and the fp16 tensor if some consumer needs it).
    Returns a list of (tensor, quantized?) aligned with `consumers`."""
    from mixdq_amd import _C
    C = x.shape[-1]
    if not (_fusable_f16(x) and x.is_contiguous() and C % 16 == 0 and C <= 2048):
        h = F.layer_norm(x, norm.normalized_shape, norm.weight, norm.bias, norm.eps)
        return [(h, False)] * len(consumers)
    groups, slot, bits = _ln_plan(norm, consumers)
    want_f16 = any(s < 0 for s in slot)
    outs, h = _C.layernorm_quantize(x, norm.weight, norm.bias, norm.eps, groups, want_f16=want_f16, _abits=bits)
    return [((outs[s], True) if s >= 0 else (h, False)) for s in slot]


def _ln_plan(norm, consumers):
    """(distinct (scale_inv, zero_point) pairs among the accelerated consumers, slot of each consumer in that
    list or -1 for one that takes the FP16 tensor, the width of each distinct quantizer) -- cached on the norm,
    re-derived when the layers change."""
    acc = [c for c in consumers if _accel(c)]
    ids = _quantizer_groups(_memo(norm), "ln", acc)
    plan = norm.__dict__.get("_mixdq_plan")
    if (plan is None or len(plan[0]) != len(consumers)
            or any(a() is not b for a, b in zip(plan[0], consumers)) or plan[3] is not ids):
        groups, slot, it = {}, [], iter(ids)   # distinct quantizers among the accelerated consumers
        for c in consumers:
            if not _accel(c):
                slot.append(-1)
                continue
            gi = next(it)
            groups.setdefault(gi, c)
            slot.append(gi)
        # weak references: a plan must not keep swapped-out float layers (and their FP16
        # weights) alive until the next forward
        plan = norm.__dict__["_mixdq_plan"] = (tuple(weakref.ref(c) for c in consumers),
                                               [_qp(groups[g]) for g in sorted(groups)], slot, ids,
                                               tuple(_abits(groups[g]) for g in sorted(groups)))
    return plan[1], plan[2], plan[4]


# the largest problem a GEMM + LayerNorm launch takes (csrc/igemm_ln.hip select_ln: one 64 x 80 or 128 x 80 tile
# per CU): M <= 4096 at N = 640, M <= 2048 at N = 1280 -- the workspace is sized for it ONCE
_LN_WS_ROWS = 4096


def _ln_workspace(owner, M, N, device):
    """The exchange buffer of the GEMM + LayerNorm launches of one network: kept on `owner` (the SDXLUNet, whose
    launches run one at a time on one stream), per device, allocated ONCE for the largest problem the launch form
    takes (2.1 MB) and never replaced -- a hipGraph captured through hip_graph_opt holds its raw pointer, so a
    buffer that grew by reallocation would leave every earlier graph writing records and counters into memory the
    allocator has handed to someone else.  The epoch in its first page only grows (launch tags); the
    departure counter is zero between launches; the third word is the sticky error word (_C.qlinear_ln_status)."""
    from mixdq_amd import _C
    store = owner.__dict__.setdefault("_ln_ws", {})
    ws = store.get(device)
    if ws is None:
        ws = store[device] = _C.qlinear_ln_workspace(max(int(M), _LN_WS_ROWS), max(int(N), 1280), device)
    need = int(_C._lib.mixdq_qlinear_ln_workspace_bytes(int(M), int(N)))
    if ws.numel() < need:      # (cannot happen for a shape the launch form takes; never silently reallocate)
        raise RuntimeError(f"GEMM + LayerNorm workspace of {ws.numel()} bytes is too small for M={M}, N={N}")
    return ws


def _gemm_res_ln(layer, x_int, residual, next_ln):
    """residual + layer(x_int) for an already quantized operand, AND -- when `next_ln` = (norm, consumers,
    owner) names the LayerNorm that reads the result -- that LayerNorm's feeds (as `_ln_feed` returns them):
    ONE launch where the GEMM + LayerNorm kernel takes the shape (mixdq_qlinear_w8a8_ln: the column tiles of
    a row block exchange their partial statistics), else the GEMM followed by the LayerNorm launch.  The
    bits are the same either way.  Returns (y, feeds or None)."""
    from mixdq_amd import _C
    if next_ln is None:
        return layer.forward_quantized(x_int, residual=residual), None
    norm, consumers, owner = next_ln
    N, K = layer.out_features, layer.in_features
    M = x_int.numel() // K
    if (not DEFUSE and _accel(layer) and _wbits(layer) == 8 and x_int.dtype == torch.int8
            and (residual is None or residual.is_contiguous())
            and norm.weight.dtype == torch.float16 and _C.qlinear_ln_supported(M, N, K)
            and all(_a8(c) for c in consumers if _accel(c))):     # (8-bit quantizers only in that launch)
        groups, slot, _ = _ln_plan(norm, consumers)
        want_f16 = any(s_ < 0 for s_ in slot)
        y, outs, h = _C.qlinear_ln(x_int, layer.weight_int, layer.scale, layer.bias0, layer.bias, residual,
                                   norm.weight, norm.bias, norm.eps, groups,
                                   _ln_workspace(owner, M, N, x_int.device), want_f16=want_f16)
        return y, [((outs[s_], True) if s_ >= 0 else (h, False)) for s_ in slot]
    y = layer.forward_quantized(x_int, residual=residual)
    return y, _ln_feed(norm, y, consumers)


def _run(layer, feed, residual=None):
    """Run a Linear on a (tensor, quantized?) feed; fold `residual` into the epilogue if possible."""
    t, quantized = feed
    if quantized:
        return layer.forward_quantized(t, residual=residual)
    if residual is not None and _fp_layer(layer) and not DEFUSE:
        return layer.forward_fp(t, residual=residual)       # FP16 kernel, add in its epilogue
    y = layer(t)
    return y if residual is None else y + residual


def _fp_layer(layer) -> bool:
    """A swapped layer on the reference's FP fallback (own FP16 kernels, residual-capable)."""
    return hasattr(layer, "forward_fp") and not getattr(layer, "valid_for_acceleration", True)


def _linear_res(layer, x, residual):
    """layer(x) + residual with the add folded into the GEMM epilogue when the layer is W8A8."""
    if _accel(layer) and _fusable_f16(x) and residual.is_contiguous():
        return layer.forward_quantized(layer._quant(x), residual=residual)
    if _fp_layer(layer) and _fusable_f16(x) and not DEFUSE:
        return layer.forward_fp(x, residual=residual)
    return layer(x) + residual


SDXL_CONFIG = dict(
    in_channels=4, out_channels=4,
    block_out_channels=(320, 640, 1280),
    layers_per_block=2,
    transformer_layers_per_block=(0, 2, 10),   # 0 = plain DownBlock2D / UpBlock2D
    mid_transformer_layers=10,
    head_dim=64,
    cross_attention_dim=2048,
    time_embed_dim=1280,
    addition_time_embed_dim=256,
    projection_class_embeddings_input_dim=2816,
    norm_num_groups=32,
)

# The SD 1.5 UNet (the reference's third model: dreamshaper-7 under LCM-LoRA, configs/stable-diffusion/lcm_lora.yaml,
# model_type 'sd'), diffusers' names for it.  What differs from SDXL besides the sizes: four levels with one
# transformer layer each (none at the innermost), EIGHT heads at every level -- heads of 40 / 80 / 160 / 160 columns
# (mid block: 160) -- no addition embedding, and 1x1 Conv2d proj_in / proj_out (use_linear_projection False).
# 859 520 964 parameters; 282 quantizable layers = 184 Linear + 98 Conv2d.
SD15_CONFIG = dict(
    in_channels=4, out_channels=4,
    block_out_channels=(320, 640, 1280, 1280),
    layers_per_block=2,
    transformer_layers_per_block=(1, 1, 1, 0),
    mid_transformer_layers=1,
    head_dim=None,
    num_attention_heads=8,             # a head COUNT per level instead of a head width: width = channels / 8
    cross_attention_dim=768,
    time_embed_dim=1280,
    addition_embed_type=None,          # no add_embedding; forward ignores added_cond_kwargs
    addition_time_embed_dim=None,
    projection_class_embeddings_input_dim=None,
    use_linear_projection=False,       # Transformer2DModel.proj_in / proj_out are 1x1 convs
    norm_num_groups=32,
)

# The SD 2.x UNet (stable-diffusion-2-1, the 768-px v-prediction model; the 512-px base model is the same network):
# SD 1.5's four levels and depths, but heads of 64 columns at every level (5 / 10 / 20 / 20 of them) instead of eight
# heads, OpenCLIP-H's 1024-wide text states, and Linear proj_in / proj_out.  Nothing in it is new to the kernels: head
# width 64 is SDXL's, and cross_attention_dim 1024 is one more K of the to_k / to_v GEMMs (K % 32 == 0, like 768 and
# 2048: every launch form takes it, no fallback).  865 910 724 parameters.  Run it with
# Sampler(..., prediction_type="v_prediction") (mixdq_amd/sampler.py).
SD21_CONFIG = dict(SD15_CONFIG, head_dim=64, num_attention_heads=None, cross_attention_dim=1024,
                   use_linear_projection=True)

# The inpainting checkpoints (stable-diffusion-xl-1.0-inpainting-0.1, stable-diffusion-inpainting): the same networks
# with a 9-channel conv_in, whose input is cat([scaled latents (4), latent-resolution mask (1), latents of the image
# with the masked pixels blanked (4)]).  The five conditioning channels are constant over a run: SDXLUNet.cond_term.
SDXL_INPAINT_CONFIG = dict(SDXL_CONFIG, in_channels=9)
SD15_INPAINT_CONFIG = dict(SD15_CONFIG, in_channels=9)

# InstructPix2Pix (timbrooks/instruct-pix2pix; diffusers' StableDiffusion[XL]InstructPix2PixPipeline): the same networks
# with an 8-channel conv_in, whose input is cat([scaled latents (4), UNSCALED latents of the image to edit (4)]).  The
# four conditioning channels are constant over a run (and zero in the unconditional rows): SDXLUNet.cond_term, fed by
# _C.ip2p_cond.  An 8-channel conv_in COULD be quantized (in_channels % 4 == 0), but the split conv_in needs it as a
# floating-point layer and refuses a quantized one: leave 'conv_in' out of the activation bit-width config of these
# UNets (it then falls back to FP16, as a 9-channel one does by itself).  859 532 484 / 2 567 475 204 parameters.
SD15_IP2P_CONFIG = dict(SD15_CONFIG, in_channels=8)
SDXL_IP2P_CONFIG = dict(SDXL_CONFIG, in_channels=8)


def head_width(cfg, channels: int) -> int:
    """Width of an attention head at a level of `channels` channels: cfg['head_dim'] (SDXL, the toy networks), or
    channels / cfg['num_attention_heads'] where the network fixes the head COUNT instead (SD 1.5)."""
    heads = cfg.get("num_attention_heads")
    if heads:
        if channels % heads:
            raise ValueError(f"{channels} channels do not split into {heads} heads")
        return channels // heads
    return cfg["head_dim"]


def _linear_proj(cfg) -> bool:
    return bool(cfg.get("use_linear_projection", True))


def sinusoidal_embedding(t: torch.Tensor, dim: int) -> torch.Tensor:
    """diffusers Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0)."""
    half = dim // 2
    key = (half, t.device)
    freqs = _SIN_FREQS.get(key)
    if freqs is None:      # a constant of (dim, device): four launches per call when recomputed
        exponent = -math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=t.device) / half
        freqs = torch.exp(exponent)
        if not (t.is_cuda and torch.cuda.is_current_stream_capturing()):
            _SIN_FREQS[key] = freqs        # (never cache a tensor that only a graph replay fills)
    emb = t.float()[:, None] * freqs[None, :]
    return torch.cat([torch.cos(emb), torch.sin(emb)], dim=-1)


_SIN_FREQS = {}


class TimestepEmbedding(nn.Module):
    def __init__(self, in_dim, dim):
        super().__init__()
        self.linear_1 = nn.Linear(in_dim, dim)
        self.linear_2 = nn.Linear(dim, dim)

    def forward(self, x):
        return self.linear_2(F.silu(self.linear_1(x)))


class ResnetBlock2D(nn.Module):
    def __init__(self, cin, cout, temb_dim, groups, split=0):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, cin, eps=1e-5)
        self.conv1 = nn.Conv2d(cin, cout, 3, 1, 1)
        self.time_emb_proj = nn.Linear(temb_dim, cout)
        self.norm2 = nn.GroupNorm(groups, cout, eps=1e-5)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1)
        self.conv_shortcut = nn.Conv2d(cin, cout, 1, 1, 0) if cin != cout else None
        self.nonlinearity = nn.SiLU()      # a MODULE, as in diffusers' ResnetBlock2D (swappable by type: nn/glue.py)
        if self.conv_shortcut is not None and split:
            # up-block: input = cat(hidden[:split], skip); the quantized shortcut uses separate
            # activation scales for the two halves (quant_block_forward_func.py:153-157)
            self.conv_shortcut.split = split

    fused = False

    def forward(self, x, temb, skip=None):
        """skip: the up-block's skip connection; the input is cat([x, skip], dim=1).  The fused
        path reads the two tensors in place (two-source GroupNorm, split shortcut) when it can."""
        if self.fused and _fusable_f16(x):
            if skip is not None and not self._pair_ok(x, skip):
                x, skip = torch.cat([x, skip], dim=1), None
            return self.forward_fused(x, temb, skip)
        if skip is not None:
            x = torch.cat([x, skip], dim=1)
        h = self.conv1(self.nonlinearity(self.norm1(x)))
        h = h + self.time_emb_proj(self.nonlinearity(temb))[:, :, None, None]
        h = self.conv2(self.nonlinearity(self.norm2(h)))
        if self.conv_shortcut is not None:
            x = self.conv_shortcut(x)
        return x + h

    def _pair_ok(self, x, skip) -> bool:
        """The (hidden, skip) pair can stay unconcatenated: the shortcut is a W8A8 split layer whose
        split is exactly `hidden`, and both tensors are channels-last with channel counts % 8."""
        sc = self.conv_shortcut
        return bool(not DEFUSE and sc is not None and getattr(sc, "valid_for_acceleration", False)
                    and getattr(sc, "split", 0) == x.shape[1] and _fusable_f16(skip)
                    and x.is_contiguous(memory_format=torch.channels_last)
                    and skip.is_contiguous(memory_format=torch.channels_last)
                    and x.shape[1] % 8 == 0 and skip.shape[1] % 8 == 0)

    def forward_fused(self, x, temb, skip=None):
        ahead = self.__dict__.pop("_t", None)
        if ahead is not None:       # projected ahead of time (SDXLUNet._project_temb_ahead)
            t, ready = ahead
            if ready is not None:
                torch.cuda.current_stream().wait_event(ready)
                t.record_stream(torch.cuda.current_stream())
        else:
            t = self.time_emb_proj(F.silu(temb))                   # [N, Cout]
        sc = None
        side = None
        if self.conv_shortcut is not None and SHORTCUT_SIDE_STREAM and skip is None:
            # the 1x1 shortcut (quantize + GEMM) only meets the main path at conv2's residual add:
            # beside norm1 / conv1 / norm2 on a side stream (A/B runs only, see above)
            main, side = torch.cuda.current_stream(), _shortcut_stream(x.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                sc = self.conv_shortcut(x)
            x.record_stream(side)
            feed, q = _gn_feed(self.norm1, x, self.conv1, silu=True)
        elif self.conv_shortcut is not None:
            # norm1's apply pass holds the block input in registers: it also writes the shortcut's
            # INT8 operand(s) -- each half of a split shortcut with its own quantizer, where it lies
            # (no concatenation) -- instead of separate quantize launches
            feed, q, raw = _gn_feed(self.norm1, x, self.conv1, silu=True, x2=skip,
                                    raw_for=self.conv_shortcut)
            if raw is not None and skip is not None:
                sc = self.conv_shortcut.forward_parts_quantized(raw[0], raw[1])
            elif raw is not None:
                sc = self.conv_shortcut.forward_quantized(raw[0])
            elif skip is not None:
                sc = self.conv_shortcut.forward_parts(x, skip)
            else:
                sc = self.conv_shortcut(x)
        else:
            feed, q = _gn_feed(self.norm1, x, self.conv1, silu=True, x2=skip)
        if q:   # h = conv1(..) + t[:, :, None, None], the add folded into the conv epilogue
            h = self.conv1.forward_quantized(feed, residual=t.contiguous(), residual_per_image=True)
        elif _fp_layer(self.conv1) and not DEFUSE:
            h = self.conv1.forward_fp(feed, residual=t.contiguous(), residual_per_image=True)
        else:
            h = self.conv1(feed) + t[:, :, None, None]
        if sc is not None:
            if side is not None:
                main.wait_stream(side)
                sc.record_stream(main)
            x = sc
        feed, q = _gn_feed(self.norm2, h, self.conv2, silu=True)
        if q and x.is_contiguous(memory_format=torch.channels_last):
            return self.conv2.forward_quantized(feed, residual=x)  # x + conv2(..)
        if not q and _fp_layer(self.conv2) and not DEFUSE:
            return self.conv2.forward_fp(feed, residual=x)
        return x + self.conv2(feed)


class Attention(nn.Module):
    def __init__(self, dim, cross_dim, head_dim):
        super().__init__()
        self.heads = dim // head_dim
        kv_dim = cross_dim if cross_dim is not None else dim
        self.to_q = nn.Linear(dim, dim, bias=False)
        self.to_k = nn.Linear(kv_dim, dim, bias=False)
        self.to_v = nn.Linear(kv_dim, dim, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(dim, dim), nn.Identity()])

    def forward(self, x, context=None):
        context = x if context is None else context
        return self.to_out[0](self.attend(self.to_q(x), self.to_k(context), self.to_v(context)))

    def attend(self, q, k, v):
        B, T, C = q.shape
        h = self.heads
        q = q.unflatten(-1, (h, C // h)).transpose(1, 2)    # views, also for column slices of a
        k = k.unflatten(-1, (h, C // h)).transpose(1, 2)    # fused q|k|v projection
        v = v.unflatten(-1, (h, C // h)).transpose(1, 2)
        o = F.scaled_dot_product_attention(q, k, v)   # FP16, as in the reference
        return o.transpose(1, 2).reshape(B, T, C)

    def cross_attend_out(self, feed_q, k, v, residual, next_ln=None):
        """residual + to_out[0](attention(to_q(feed_q), k, v)) for the cross-attention, whose keys /
        values (77 text tokens) fit one workgroup's LDS: to_q's INT8 GEMM, the attention core and
        to_out.0's quantizer are ONE launch; q never exists in memory.  Bit-identical to the
        three-step path it replaces (tests/test_fused_gpu.py)."""
        if _cross_fusable(self, feed_q, k, v, residual):
            from mixdq_amd import _C
            q, out = self.to_q, self.to_out[0]
            o_int = _C.qlinear_attention(feed_q[0], q.weight_storage()[0],
                                         q.scale, q.bias0, k, v, *_qp(out), **q._wkw(), _abits=_abits(out))
            return _gemm_res_ln(out, o_int, residual, next_ln)
        return self.attend_out(_run(self.to_q, feed_q), k, v, residual, next_ln=next_ln)

    def attend_out(self, q, k, v, residual, prefetch=None, next_ln=None):
        """residual + to_out[0](attention(q, k, v)) on the fused path: the HIP FP16 attention core
        reads q/k/v in place (column slices of the fused projection included) and, when to_out[0]
        is W8A8, emits its INT8 operand directly; the residual add rides in the GEMM epilogue."""
        from mixdq_amd import _C
        out = self.to_out[0]
        C = q.shape[-1]
        D = C // self.heads
        from mixdq_amd.nn.glue import ATTENTION_HEAD_DIMS      # the UNets' widths (INT8 output; not the VAE's 512)
        ok = (C == self.heads * D and D in ATTENTION_HEAD_DIMS
              and all(_fusable_f16(t) and t.dim() == 3 and t.stride(-1) == 1
                      and t.stride(0) % 8 == 0 and t.stride(1) % 8 == 0
                      and t.data_ptr() % 16 == 0 for t in (q, k, v)))
        def plain(y):          # (y, feeds of the LayerNorm that reads y) by two launches
            return y, (None if next_ln is None else _ln_feed(next_ln[0], y, next_ln[1]))
        if not ok:
            return plain(_linear_res(out, self.attend(q, k, v), residual))
        sc = None if D == 64 else D ** -0.5          # (SDPA's default scale, as in attend)
        if _accel(out) and residual.is_contiguous():
            o_int = _C.attention_f16(q, k, v, self.heads, *_qp(out), softmax_scale=sc, _prefetch=prefetch,
                                     _abits=_abits(out))
            return _gemm_res_ln(out, o_int, residual, next_ln)
        return plain(_linear_res(out, _C.attention_f16(q, k, v, self.heads, softmax_scale=sc, _prefetch=prefetch),
                                 residual))


CROSS_FUSE_MAX_ROWS = int(__import__("os").environ.get("MIXDQ_CROSS_FUSE_MAX_ROWS", "4096"))
# LayerNorms in the epilogue of the GEMM that produces their input (csrc/igemm_ln.hip).  Off by default: the step
# time is EQUAL either way (10.975 / 10.986 ms with, 10.965 / 10.945 without, same box: DESIGN.md section 3.13) -- 151
# launches fewer, paid for by a cross-workgroup exchange per launch -- and the plain form keeps every launch free of
# inter-workgroup waits.  MIXDQ_LN_CHAIN=1 (or `mixdq_amd.unet.LN_CHAIN = True`) turns it on; bench.py times both.
LN_CHAIN = __import__("os").environ.get("MIXDQ_LN_CHAIN", "0") == "1"
# weight prefetch from the self-attention launch: on for launches of up to this many rows
PREFETCH = __import__("os").environ.get("MIXDQ_PREFETCH", "1") != "0"
WEIGHT_ARENA = __import__("os").environ.get("MIXDQ_WEIGHT_ARENA", "0") == "1"      # arena.py (prepare_fused_)
PREFETCH_MAX_ROWS = int(__import__("os").environ.get("MIXDQ_PREFETCH_MAX_ROWS", "0"))      # 0: no limit (see _build_prefetch_plan)
PREFETCH_MB_PER_LAUNCH = float(__import__("os").environ.get("MIXDQ_PREFETCH_MB", "48"))   # per 1024 x 1024 scores
PREFETCH_MAX_LEAD = int(__import__("os").environ.get("MIXDQ_PREFETCH_LEAD", "4"))         # launches a weight may be read ahead
PREFETCH_SKIP_MB = float(__import__("os").environ.get("MIXDQ_PREFETCH_SKIP_MB", "0"))       # experiment: leave tensors above this cold (0: off)


def _trace_signature(trace):
    return tuple(it if isinstance(it, tuple) else (it.data_ptr(), it.numel()) for it in trace)


def _plan_alive(plan, device) -> bool:
    """Every tensor of the plan still exists, at the address it was planned at, on `device`."""
    for lst in plan["lists"]:
        for ref, ptr in zip(lst, plan["ptrs"][id(lst)]):
            t = ref()
            if t is None or t.device != device or t.data_ptr() != ptr:
                return False
    return True


def _build_prefetch_plan(trace):
    """Which weights does each self-attention launch of a forward read ahead (mixdq_attention_f16_prefetch)?
    `trace` (mixdq_amd._C.PrefetchContext.trace) is the forward's execution order: weight operands as the GEMM / conv entry
    points saw them, and a marker (rows, keys) per long-key attention launch.  Launch j is given the weights
    used between it and launch j + 1 -- the rest of its transformer block, the next block's q|k|v; at the
    end of a Transformer2DModel also proj_out, the ResNet convs, shortcuts and samplers up to the next
    transformer -- up to a byte budget proportional to the launch's own work (it should not outlast the
    attention) and 16 ranges; what does not fit is offered to launch j - 1, ... j - PREFETCH_MAX_LEAD behind
    THEIR own intervals (read earlier still: the 256 MB Infinity Cache keeps a few hundred microseconds of
    the step's weight stream, not more -- an unbounded cascade measured slower than no look-back at all),
    and stays cold if none of them has room.  MIXDQ_PREFETCH_MAX_ROWS (default 0: off) leaves launches of more
    rows without a payload: from batch 2 on the attention launch fills the chip, so its payload workgroups run in
    the launch's tail and lengthen it -- measured, the weights they leave in the cache are still worth more
    (batch 8: 48.65 -> 47.98 ms, batch 2: 17.17 -> 16.98, batch 4: 27.73 -> 27.60; 4096 was the first default).
    Weights used before the first attention launch have no host and stay cold."""
    marks = [(i, it) for i, it in enumerate(trace) if isinstance(it, tuple)]
    if not marks:
        return None
    lists = [[] for _ in marks]
    carry = []                                       # (tensor, launches it has been moved back)
    nbytes = lambda t: t.numel() * t.element_size()  # noqa: E731
    for j in range(len(marks) - 1, -1, -1):
        lo = marks[j][0] + 1
        hi = marks[j + 1][0] if j + 1 < len(marks) else len(trace)
        own, seen = [], set()
        for t in trace[lo:hi]:
            if isinstance(t, tuple) or t.data_ptr() in seen or nbytes(t) < (64 << 10):
                continue
            if PREFETCH_SKIP_MB and nbytes(t) > PREFETCH_SKIP_MB * 1e6:
                continue
            seen.add(t.data_ptr())
            own.append(t)
        _, rows, keys = marks[j][1]
        budget = (0 if PREFETCH_MAX_ROWS and rows > PREFETCH_MAX_ROWS
                  else PREFETCH_MB_PER_LAUNCH * 1e6 * rows * keys / float(1 << 20))
        budget = min(budget, 160e6)
        new_carry, blocked = [], False
        for t in own:                                # the launch's own interval first, in order
            if not blocked and nbytes(t) <= budget and len(lists[j]) < 16:
                lists[j].append(t)
                budget -= nbytes(t)
            else:
                blocked = True
                new_carry.append((t, 1))
        for t, d in carry:                           # then what later launches could not take
            if t.data_ptr() in seen:
                continue
            seen.add(t.data_ptr())
            if nbytes(t) <= budget and len(lists[j]) < 16:
                lists[j].append(t)
                budget -= nbytes(t)
            elif d < PREFETCH_MAX_LEAD:
                new_carry.append((t, d + 1))         # else: stays cold
        carry = new_carry
    import weakref
    ref_lists = [[weakref.ref(t) for t in lst] for lst in lists]       # never keeps a replaced weight alive
    ptrs = {id(rl): [t.data_ptr() for t in lst] for rl, lst in zip(ref_lists, lists)}
    return {"lists": ref_lists, "ptrs": ptrs, "sig": _trace_signature(trace)}


def _cross_fusable(attn, feed, k, v, residual) -> bool:
    """to_q + cross-attention + quantize for to_out.0 as ONE launch (mixdq_qlinear_w8a8_attn)?"""
    from mixdq_amd import _C
    q, out = attn.to_q, attn.to_out[0]
    t, quantized = feed
    return bool(not DEFUSE and quantized and _accel(q) and q.bias is None and _accel(out) and t.dim() == 3
                and attn.heads * 64 == q.out_features and residual.is_contiguous()
                and all(_fusable_f16(z) and z.dim() == 3 and z.stride(-1) == 1
                        and z.stride(0) % 8 == 0 and z.stride(1) % 8 == 0
                        and z.data_ptr() % 16 == 0 for z in (k, v))
                and k.shape == v.shape and k.shape[0] == t.shape[0]
                # the fused launch runs the GEMM on 64 x 128 tiles: from a few thousand rows on, the
                # large-tile GEMM + the attention kernel are faster (batch 8: 26 + 20 us vs 56 us)
                and t.shape[0] * t.shape[1] <= CROSS_FUSE_MAX_ROWS
                and _C.qlinear_attention_supported(t.shape, q.out_features, q.in_features, k))


class GEGLU(nn.Module):
    def __init__(self, dim, inner):
        super().__init__()
        self.proj = nn.Linear(dim, inner * 2)

    def forward(self, x):
        x, gate = self.proj(x).chunk(2, dim=-1)
        return x * F.gelu(gate)


class FeedForward(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.net = nn.ModuleList([GEGLU(dim, dim * 4), nn.Identity(), nn.Linear(dim * 4, dim)])

    def forward(self, x):
        assert not self.__dict__.get("_interleaved"), "rows are interleaved: fused path only"
        return self.net[2](self.net[0](x))

    def set_interleaved(self, on: bool):
        """Store ff.net.0.proj's rows as value|gate groups of 16 (on) or in the ordinary
        [values | gates] order (off).  Interleaved, one GEMM launch produces net.2's INT8 operand
        (GEMM + GEGLU + quantize); only pairs whose net.2 has an 8-bit activation quantizer qualify (that
        launch refuses a 4-bit one: net.2 then gets its operand from the stand-alone GEGLU launch)."""
        from mixdq_amd import _C
        proj, out_layer = self.net[0].proj, self.net[2]
        have = bool(self.__dict__.get("_interleaved"))
        if on == have:
            return
        if on and not (_accel(proj) and _accel(out_layer) and _a8(out_layer) and proj.out_features % 64 == 0
                       and proj.in_features % 16 == 0 and proj.weight_scales.is_cuda):
            return
        perm = _C.geglu_row_order(proj.out_features // 2, proj.weight_scales.device)
        if not on:
            perm = torch.argsort(perm)
        proj.permute_output_rows_(perm)
        self.__dict__["_interleaved"] = on

    def forward_fused(self, feed, residual, next_ln=None):
        """residual + net2(geglu(proj(feed))): GEGLU fused with net.2's quantizer, the residual add
        folded into net.2's epilogue.  With `next_ln` (the LayerNorm that reads the result: the next
        block's norm1) returns (y, that LayerNorm's feeds), the LayerNorm riding in net.2's launch where
        the GEMM + LayerNorm kernel takes the shape (`_gemm_res_ln`)."""
        from mixdq_amd import _C
        out_layer = self.net[2]
        if next_ln is not None:
            y = self.forward_fused(feed, residual) if (DEFUSE or not self.__dict__.get("_interleaved")) else None
            if y is not None:
                return y, _ln_feed(next_ln[0], y, next_ln[1])
            assert feed[1], "interleaved rows need the quantized feed"
            q = self.net[0].proj.forward_quantized_geglu(feed[0], out_layer)
            return _gemm_res_ln(out_layer, q, residual, next_ln)
        if self.__dict__.get("_interleaved") and not DEFUSE:
            assert feed[1], "interleaved rows need the quantized feed"
            q = self.net[0].proj.forward_quantized_geglu(feed[0], out_layer)
            return out_layer.forward_quantized(q, residual=residual)
        h = _run(self.net[0].proj, feed)
        if self.__dict__.get("_interleaved"):     # DEFUSE: columns back to [values | gates]
            D2 = h.shape[-1]
            inv = torch.argsort(_C.geglu_row_order(D2 // 2, h.device))
            h = h.index_select(-1, inv)
        D = h.shape[-1] // 2
        if _fusable_f16(h) and h.is_contiguous() and D % 8 == 0:
            if _accel(out_layer):
                q, _ = _C.geglu_quantize(h, *_qp(out_layer), _abits=_abits(out_layer))
                return out_layer.forward_quantized(q, residual=residual)
            _, g = _C.geglu_quantize(h, want_f16=True)
            return _run(out_layer, (g, False), residual)
        a, gate = h.chunk(2, dim=-1)
        return out_layer(a * F.gelu(gate)) + residual


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim, cross_dim, head_dim):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn1 = Attention(dim, None, head_dim)
        self.norm2 = nn.LayerNorm(dim)
        self.attn2 = Attention(dim, cross_dim, head_dim)
        self.norm3 = nn.LayerNorm(dim)
        self.ff = FeedForward(dim)

    fused = False

    def forward(self, x, context):
        if self.fused and _fusable_f16(x):
            return self.forward_fused(x, context)
        x = x + self.attn1(self.norm1(x))
        x = x + self.attn2(self.norm2(x), context)
        return x + self.ff(self.norm3(x))

    def _qkv_fused(self):
        """Self-attention to_q / to_k / to_v read the same normalised tensor; when all three are
        W8A8 with the SAME activation quantizer (they are calibrated on the same data) and carry no
        bias, one GEMM against the row-concatenated weights [3C, C] replaces three: per-channel
        scale / bias0 simply concatenate, so every output element is computed exactly as before
        (`_pack_rows`).  Nothing negative is cached: the decision is re-taken whenever the layers
        or their quantizer tensors change (e.g. quantize_unet after an FP16 run of this graph)."""
        a = self.attn1
        layers = [a.to_q, a.to_k, a.to_v]
        if DEFUSE or not all(_accel(m) and m.bias is None for m in layers):
            return None
        if len(set(_quantizer_groups(_memo(self), "qkv", layers))) != 1:
            return None
        if not _uniform_storage(layers):
            return None
        pack = self.__dict__.get("_qkv")
        if not _pack_valid(pack, layers):
            pack = self.__dict__["_qkv"] = _pack_rows(layers)
        return pack

    def ln1_consumers(self):
        a = self.attn1
        return [a.to_q, a.to_k, a.to_v]

    def forward_fused(self, x, context, feeds1=None, next_ln=None, owner=None):
        """`feeds1`: norm1's feeds when the GEMM that produced x already computed them (`_gemm_res_ln`);
        `next_ln`: the LayerNorm that reads this block's output (the next block's norm1) -- then returns
        (x, its feeds); `owner`: the module that keeps the GEMM + LayerNorm exchange buffer (None: the
        LayerNorms of this block run as launches of their own)."""
        x = x.contiguous()
        a = self.attn1
        pack = self._qkv_fused()
        feeds = feeds1 if feeds1 is not None else _ln_feed(self.norm1, x, self.ln1_consumers())
        ln2 = None if owner is None else (self.norm2, [self.attn2.to_q], owner)
        ln3 = None if owner is None else (self.norm3, [self.ff.net[0].proj], owner)
        if pack is not None and feeds[0][1]:
            from mixdq_amd.op.qlinear import qlinear
            q0 = a.to_q
            qkv = qlinear(feeds[0][0], pack["w"], pack["wscale"], q0.act_scales, q0.act_zero_points,
                          pack["wsum"], pack["scale"], pack["bias0"], None, _w4=pack["w4"],
                          _w2=pack.get("w2", False))
            C = pack["C"]
            x, f2 = a.attend_out(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], x, next_ln=ln2)
        else:
            fq, fk, fv = feeds                                      # x + attn1(norm1(x))
            x, f2 = a.attend_out(_run(a.to_q, fq), _run(a.to_k, fk), _run(a.to_v, fv), x, next_ln=ln2)
        a = self.attn2
        (fq,) = f2 if f2 is not None else _ln_feed(self.norm2, x, [a.to_q])
        kv = self.__dict__.pop("_kv", None)
        if kv is not None:          # projected ahead of time (SDXLUNet._project_context_ahead)
            k, v, ready = kv
            if ready is not None:
                torch.cuda.current_stream().wait_event(ready)
                k.record_stream(torch.cuda.current_stream())
                v.record_stream(torch.cuda.current_stream())
        else:
            k, v = a.to_k(context), a.to_v(context)                 # K/V: BOS path
        x, f3 = a.cross_attend_out(fq, k, v, x, next_ln=ln3)        # x + attn2(norm2(x), ctx)
        (ff,) = f3 if f3 is not None else _ln_feed(self.norm3, x, [self.ff.net[0].proj])
        if next_ln is None:
            return self.ff.forward_fused(ff, x)                     # x + ff(norm3(x))
        return self.ff.forward_fused(ff, x, next_ln=next_ln)        # ... and the next block's norm1 feeds


def _proj_rows(conv, feed, bhw, residual=None):
    """A 1x1 Conv2d proj_in / proj_out of a Transformer2DModel on token rows: `feed` = (tensor, quantized?) as rows
    [B, HW, C] -- the NHWC memory of the image -- returns rows [B, HW, N] (+ `residual`, rows too).  Over those rows
    the 1x1 conv IS a Linear, and a W8A8 layer runs as one: the INT8 GEMM entry point on the [N, C] view of the
    conv's KRSC weight, the residual in its epilogue (no conv path is involved).  Any other layer (FP16 network,
    FP fallback, de-fused reference) is called as the module it is, on the image view of the same memory."""
    t, quantized = feed
    B, H, W = bhw
    if (getattr(conv, "valid_for_acceleration", False) and conv.split == 0 and not conv.w_packed4
            and (quantized or _fusable_f16(t)) and (quantized or not DEFUSE)):
        from mixdq_amd.op.qlinear import qlinear
        from mixdq_amd.nn.Conv2d import quant_op
        x_int = t if quantized else quant_op(t, *_qp(conv))
        w = conv.weight_int
        w2 = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)              # [N, C]: a view of the KRSC storage
        fold = residual is not None and residual.is_contiguous() and not DEFUSE
        y = qlinear(x_int, w2, conv.weight_scales, conv.act_scales, conv.act_zero_points, conv.bias0, conv.scale,
                    conv.bias0, conv.bias, _residual=residual if fold else None)
        return y if residual is None or fold else y + residual
    img = t.reshape(B, H, W, t.shape[-1]).permute(0, 3, 1, 2)            # [B, C, H, W], channels-last in memory
    y = conv(img).permute(0, 2, 3, 1).reshape(B, H * W, -1)
    return y if residual is None else y + residual


class Transformer2DModel(nn.Module):
    def __init__(self, dim, depth, cross_dim, head_dim, groups, linear_proj=True):
        super().__init__()
        self.norm = nn.GroupNorm(groups, dim, eps=1e-6)
        # diffusers' use_linear_projection: Linear on the token rows (SDXL), or a 1x1 Conv2d on the image (SD 1.5:
        # weights [C, C, 1, 1]) -- the same arithmetic, applied before / after the image <-> tokens reshape
        self.proj_in = nn.Linear(dim, dim) if linear_proj else nn.Conv2d(dim, dim, 1, 1, 0)
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(dim, cross_dim, head_dim) for _ in range(depth)])
        self.proj_out = nn.Linear(dim, dim) if linear_proj else nn.Conv2d(dim, dim, 1, 1, 0)
        self.linear_proj = bool(linear_proj)

    fused = False

    def forward(self, x, context):
        B, C, H, W = x.shape
        res = x
        if self.fused and _fusable_f16(x) and x.is_contiguous(memory_format=torch.channels_last):
            feed, q = _gn_feed(self.norm, x, self.proj_in, silu=False)
            feed = feed.permute(0, 2, 3, 1).reshape(B, H * W, C)    # NHWC memory == [B, HW, C]
            blocks = list(self.transformer_blocks)
            owner = self.__dict__.get("_ln_owner")
            chain = (LN_CHAIN and owner is not None and not DEFUSE and blocks
                     and all(getattr(b, "fused", False) for b in blocks))
            if chain:
                # every LayerNorm rides in the launch of the GEMM that produces its input (round 5):
                # proj_in -> block 0's norm1, attn1.to_out.0 -> norm2, attn2.to_out.0 -> norm3,
                # ff.net.2 -> the next block's norm1
                first = (blocks[0].norm1, blocks[0].ln1_consumers(), owner)
                if not self.linear_proj:       # (a conv projection keeps its own launch: the chain starts behind it)
                    h, feeds = _proj_rows(self.proj_in, (feed, q), (B, H, W)), None
                elif q and _accel(self.proj_in):
                    h, feeds = _gemm_res_ln(self.proj_in, feed, None, first)
                else:
                    h = _run(self.proj_in, (feed, q))
                    feeds = None
                for i, blk in enumerate(blocks):
                    nxt = blocks[i + 1] if i + 1 < len(blocks) else None
                    nl = None if nxt is None else (nxt.norm1, nxt.ln1_consumers(), owner)
                    out = blk.forward_fused(h, context, feeds1=feeds, next_ln=nl, owner=owner)
                    h, feeds = out if nl is not None else (out, None)
            else:
                h = _run(self.proj_in, (feed, q)) if self.linear_proj else _proj_rows(self.proj_in, (feed, q), (B, H, W))
                for blk in blocks:
                    h = blk(h, context)
            res_rows = res.permute(0, 2, 3, 1).reshape(B, H * W, C)
            if self.linear_proj:
                h = _linear_res(self.proj_out, h, res_rows)         # proj_out(h) + res
            else:
                h = _proj_rows(self.proj_out, (h, False), (B, H, W), residual=res_rows)
            return h.reshape(B, H, W, C).permute(0, 3, 1, 2)
        if not self.linear_proj:
            # diffusers with use_linear_projection False: norm -> conv -> tokens; tokens -> conv -> + residual
            h = self.proj_in(self.norm(x))
            h = h.permute(0, 2, 3, 1).reshape(B, H * W, C)
            for blk in self.transformer_blocks:
                h = blk(h, context)
            h = h.reshape(B, H, W, C).permute(0, 3, 1, 2)
            return self.proj_out(h) + res
        h = self.norm(x).permute(0, 2, 3, 1).reshape(B, H * W, C)   # free when channels-last
        h = self.proj_in(h)
        for blk in self.transformer_blocks:
            h = blk(h, context)
        h = self.proj_out(h)
        h = h.reshape(B, H, W, C).permute(0, 3, 1, 2)               # channels-last view
        return h + res


class Downsample2D(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 2, 1)

    def forward(self, x):
        return self.conv(x)


class Upsample2D(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 1, 1)

    fused = False

    def forward(self, x):
        conv = self.conv
        if (self.fused and not DEFUSE and _fusable_f16(x) and _accel(conv)
                and x.is_contiguous(memory_format=torch.channels_last)
                and conv.upsample2x_supported(tuple(x.shape))):
            # quantizing commutes with nearest upsampling: quantize the SMALL tensor, and let the
            # conv's halo loader read pixel (y / 2, x / 2) -- no upsampled tensor, fp16 or int8
            from mixdq_amd.nn.Conv2d import quant_op
            return conv.forward_quantized(quant_op(x, *_qp(conv)), upsample2x=True)
        return self.conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))


class DownBlock(nn.Module):
    def __init__(self, cin, cout, temb, n_layers, depth, cfg, add_down):
        super().__init__()
        self.resnets = nn.ModuleList(
            [ResnetBlock2D(cin if i == 0 else cout, cout, temb, cfg["norm_num_groups"])
             for i in range(n_layers)])
        if depth:
            self.attentions = nn.ModuleList(
                [Transformer2DModel(cout, depth, cfg["cross_attention_dim"], head_width(cfg, cout),
                                    cfg["norm_num_groups"], _linear_proj(cfg)) for _ in range(n_layers)])
        self.has_attn = bool(depth)
        if add_down:
            self.downsamplers = nn.ModuleList([Downsample2D(cout)])
        self.has_down = add_down

    def forward(self, x, temb, context):
        outs = []
        for i, res in enumerate(self.resnets):
            x = res(x, temb)
            if self.has_attn:
                x = self.attentions[i](x, context)
            outs.append(x)
        if self.has_down:
            x = self.downsamplers[0](x)
            outs.append(x)
        return x, outs


class MidBlock(nn.Module):
    def __init__(self, c, temb, depth, cfg):
        super().__init__()
        self.attentions = nn.ModuleList(
            [Transformer2DModel(c, depth, cfg["cross_attention_dim"], head_width(cfg, c),
                                cfg["norm_num_groups"], _linear_proj(cfg))])
        self.resnets = nn.ModuleList([ResnetBlock2D(c, c, temb, cfg["norm_num_groups"])
                                      for _ in range(2)])

    def forward(self, x, temb, context):
        x = self.resnets[0](x, temb)
        x = self.attentions[0](x, context)
        return self.resnets[1](x, temb)


class UpBlock(nn.Module):
    def __init__(self, prev_c, cout, skip_channels, temb, depth, cfg, add_up):
        super().__init__()
        res = []
        for i, skip in enumerate(skip_channels):
            hidden = prev_c if i == 0 else cout
            res.append(ResnetBlock2D(hidden + skip, cout, temb, cfg["norm_num_groups"],
                                     split=hidden))
        self.resnets = nn.ModuleList(res)
        if depth:
            self.attentions = nn.ModuleList(
                [Transformer2DModel(cout, depth, cfg["cross_attention_dim"], head_width(cfg, cout),
                                    cfg["norm_num_groups"], _linear_proj(cfg)) for _ in skip_channels])
        self.has_attn = bool(depth)
        if add_up:
            self.upsamplers = nn.ModuleList([Upsample2D(cout)])
        self.has_up = add_up

    def forward(self, x, skips, temb, context):
        for i, res in enumerate(self.resnets):
            x = res(x, temb, skips.pop())      # input = cat([x, skip], dim=1)
            if self.has_attn:
                x = self.attentions[i](x, context)
        if self.has_up:
            x = self.upsamplers[0](x)
        return x


class FusedGraph(nn.Module):
    """What a network made of this file's blocks needs for the fused graph, whichever blocks it has -- the UNet, or a
    ControlNet (its encoder half, mixdq_amd/controlnet.py): prepare_fused_ / set_fused, the time-embedding and context
    projections issued ahead of the blocks, the holder of weight-derived tensors, the weight-prefetch plan, the
    embedding of (timestep, added conditions) and conv_in's with-term form.  Everything here walks self.modules();
    a subclass has `cfg`, `conv_in`, `time_embedding` and, where the config asks for it, `add_embedding`."""
    fused = False

    def _grouped(self, name, key, members, wbits):
        """Cached device table of a grouped launch (rebuilt when any member's storage changed).
        `wbits`: the members' weight storage, 8 / 4 / 2 bits."""
        from mixdq_amd._C import GemmGroupTable
        tables = self.__dict__.setdefault("_group_tables", {})
        want = tuple(m[0].data_ptr() for m in members) + tuple(m[4].data_ptr() for m in members)
        t = tables.get((name, key))
        if t is None or t.key != want or t.wbits != wbits:
            t = tables[(name, key)] = GemmGroupTable(members, wbits=wbits)
        return t

    def _project_context_ahead(self, context):
        """Cross-attention keys / values depend only on the text embeddings, not on the latent: in
        the fused graph all 2 x 70 to_k / to_v projections are issued up front -- as ONE grouped
        launch per activation quantizer (gridDim.y = block; 367 MB of weights streamed at HBM rate
        instead of 70 latency-bound launches), each writing its block's persistent [B, T, 2C] buffer
        whose BOS row is a constant.  The INT8 copy of the context (tokens 1.., BOS carve-out) is
        shared by every layer whose activation quantizer is identical.  (Round 1 ran these on a
        side stream; measured, a second long-lived branch in the hipGraph costs more than the
        kernels it hides: 14.96 -> 14.36 ms with both side branches removed.)"""
        from mixdq_amd.nn.glue import kept_bos_buffer
        blocks = [m for m in self.modules() if isinstance(m, BasicTransformerBlock)]
        if not blocks or not context.is_cuda:
            return
        f16_tail = context.dtype == torch.float16 and context.shape[1] > 1
        B, T = context.shape[0], context.shape[1]

        def bos_w8a8(layer):
            return bool(getattr(layer, "valid_for_acceleration", False)
                        and getattr(layer, "bos", False) and f16_tail)

        # quantizer grouping of every BOS W8A8 K/V layer, taken once (memoised; no host
        # comparison ever runs inside the forward proper, so the loop below is capture-safe)
        kv_layers = [l for blk in blocks for l in (blk.attn2.to_k, blk.attn2.to_v) if bos_w8a8(l)]
        gid = dict(zip(map(id, kv_layers), _quantizer_groups(_memo(self), "ctx", kv_layers)))
        shared = {}                       # quantizer group -> int8 context (tokens 1..)

        def ctx_int8(layer):
            g = gid[id(layer)]
            if g not in shared:          # (the group is the quantizer AND its width)
                shared[g] = layer._quant(context[:, 1:, :])
            return shared[g]

        grouped = {}                      # (quantizer group, K, w4) -> [(block, pack)]
        for blk in blocks:
            lk, lv = blk.attn2.to_k, blk.attn2.to_v
            pack = None
            if bos_w8a8(lk) and bos_w8a8(lv) and gid[id(lk)] == gid[id(lv)]:
                pack = self._kv_pack(blk, context)
            if pack is not None:        # to_k | to_v as ONE GEMM against [2C, K] (cf. _qkv_fused)
                # persistent [B, T, 2C] buffer PER SHAPE (a captured graph keeps raw pointers into
                # it: a buffer is never dropped while its pack lives), BOS row derived from the two BOS tensors
                o = kept_bos_buffer(pack.setdefault("outs", {}), (B, T, context.device), 2 * pack["C"],
                                    (lk.bos_pre_computed, lv.bos_pre_computed))
                blk._kv = (o[..., :pack["C"]], o[..., pack["C"]:], None)
                grouped.setdefault((gid[id(lk)], lk.in_features, pack["wbits"]), []).append(
                    (lk, pack, o))
                continue
            outs = []
            for layer in (lk, lv):
                if not bos_w8a8(layer):
                    outs.append(layer(context))
                    continue
                # persistent K / V buffer per layer and shape (never dropped: see above)
                buf = kept_bos_buffer(layer.__dict__.setdefault("_kv_buf", {}), (B, T, context.device),
                                      layer.out_features, (layer.bos_pre_computed,))
                outs.append(layer.forward_bos_quantized(ctx_int8(layer), B, T, out=buf))
            blk._kv = (outs[0], outs[1], None)
        from mixdq_amd import _C
        from mixdq_amd.op.qlinear import qlinear
        for (g, K, wb), members in grouped.items():
            lk0 = members[0][0]
            x_int = ctx_int8(lk0)
            if len(members) == 1:
                pack, o = members[0][1], members[0][2]
                qlinear(x_int, pack["w"], pack["wscale"], lk0.act_scales, lk0.act_zero_points,
                        pack["wsum"], pack["scale"], pack["bias0"], None, _out=o,
                        _row_map=(T - 1, T, 1), _w4=wb == 4, _w2=wb == 2)
                continue
            table = self._grouped("kv", (g, K, wb, B, T), [
                (pk["w"], pk["bias0"], pk["scale"], None, o) for _, pk, o in members], wb)
            _C.qlinear_grouped(x_int, table, _row_map=(T - 1, T, 1))

    @staticmethod
    def _kv_pack(blk, context=None):
        """Cross-attention to_k / to_v read the same tokens; when both are W8A8 BOS layers with the
        same activation quantizer and no bias, one GEMM against the row-concatenated weights
        replaces two (`_pack_rows`: every output element is computed exactly as before)."""
        lk, lv = blk.attn2.to_k, blk.attn2.to_v
        layers = [lk, lv]
        if not (all(getattr(m, "valid_for_acceleration", False) and getattr(m, "bos", False)
                    and m.bias is None for m in layers)
                and lk.out_features == lv.out_features):
            return None
        if context is not None and not (context.dtype == torch.float16 and context.shape[1] > 1):
            return None
        if len(set(_quantizer_groups(_memo(blk), "kv", layers))) != 1:
            return None
        if not _uniform_storage(layers):
            return None                         # mixed int8 / packed storage: see prepare_fused_
        pack = blk.__dict__.get("_kvpack")
        if not _pack_valid(pack, layers):
            pack = blk.__dict__["_kvpack"] = _pack_rows(layers)
        return pack

    def _project_temb_ahead(self, emb):
        """Every ResnetBlock2D adds time_emb_proj(silu(emb)): 22 M = batch GEMMs (plus their SiLU
        and quantize launches) that depend only on the time embedding.  In the fused graph they
        are issued up front: SiLU once, one INT8 copy per distinct activation quantizer (the layers
        are all calibrated on this same tensor) and ONE grouped launch for all layers that share
        it (gridDim.y = layer; N differs per layer), into persistent [B, Cout] buffers."""
        resnets = [m for m in self.modules() if isinstance(m, ResnetBlock2D)]
        if not resnets or not emb.is_cuda:
            return
        s = F.silu(emb)
        B = s.shape[0]
        acc = [r.time_emb_proj for r in resnets if _accel(r.time_emb_proj)]
        ok = _fusable_f16(s) and s.dim() == 2
        gid = dict(zip(map(id, acc), _quantizer_groups(_memo(self), "temb", acc)))
        shared, grouped = {}, {}
        for res in resnets:
            layer = res.time_emb_proj
            if not (_accel(layer) and ok):
                res._t = (layer(s), None)
                continue
            # persistent output per batch size: a graph captured at another batch keeps raw
            # pointers to ITS buffer, so none is ever dropped or reused for a different shape
            bufs = layer.__dict__.setdefault("_t_out", {})
            buf = bufs.get((B, s.device))
            if buf is None:
                buf = bufs[(B, s.device)] = torch.empty((B, layer.out_features),
                                                        dtype=torch.float16, device=s.device)
            res._t = (buf, None)
            grouped.setdefault((gid[id(layer)], layer.in_features, _wbits(layer)),
                               []).append((layer, buf))
        from mixdq_amd import _C
        for (g, K, wb), members in grouped.items():
            if g not in shared:
                shared[g] = members[0][0]._quant(s)
            x_int = shared[g]
            if len(members) == 1:
                members[0][0]._gemm(x_int, out=members[0][1])
                continue
            table = self._grouped("temb", (g, K, wb, B), [
                (m.weight_storage()[0], m.bias0, m.scale, m.bias, buf)
                for m, buf in members], wb)
            _C.qlinear_grouped(x_int, table)

    def refresh_derived_(self):
        """After buffers were written IN PLACE (load_state_dict, shard.broadcast_module_state): every derived
        tensor of this network follows at its address, so that captured graphs see the new values too."""
        for m in self.modules():
            if m is not self and hasattr(m, "refresh_derived_"):
                m.refresh_derived_()
            d = m.__dict__
            kept = (d.get("_kv_buf"), d.get("_mixdq_bos_out"), (d.get("_kvpack") or {}).get("outs"))
            for slot in [s for bufs in kept if bufs for s in bufs.values()]:
                derived.refresh(slot[1])           # (the BOS row of a kept K / V buffer)
        derived.refresh(self.__dict__.get("_derived_tensors"))
        return self

    def prepare_fused_(self):
        """Explicit post-conversion step of the fused graph (called by `set_fused(True)`): whatever
        changes a module's BUFFERS happens here, once, never inside a forward -- mixed int8 / packed
        4-bit q|k|v and k|v groups are widened to one storage kind (`unify_packed_storage_`) and
        their row-concatenated GEMM operands are built (`_pack_rows`: the layers' buffers become
        views of the pack).  After it, state-dict keys and shapes are final: a checkpoint saved now
        loads strictly later, and every rank holds the same set of buffers before
        `shard.broadcast_module_state`."""
        for blk in self.modules():
            if not isinstance(blk, BasicTransformerBlock):
                continue
            a = blk.attn1
            qkv = [a.to_q, a.to_k, a.to_v]
            if (all(_accel(m) and m.bias is None for m in qkv)
                    and len(set(_quantizer_groups(_memo(blk), "qkv", qkv))) == 1
                    and unify_packed_storage_(qkv)):
                blk._qkv_fused()
            kv = [blk.attn2.to_k, blk.attn2.to_v]
            if (all(getattr(m, "valid_for_acceleration", False) and getattr(m, "bos", False)
                    and m.bias is None for m in kv)
                    and kv[0].out_features == kv[1].out_features
                    and len(set(_quantizer_groups(_memo(blk), "kv", kv))) == 1
                    and unify_packed_storage_(kv)):
                self._kv_pack(blk)
        for m in self.modules():            # the network that keeps the GEMM + LayerNorm exchange buffer
            if isinstance(m, Transformer2DModel):
                m.__dict__["_ln_owner"] = self
        # the GELU table of the GEMM+GEGLU launches is built here, eagerly: a first use inside a stream
        # capture could only RECORD its init kernel into that graph (csrc/igemm_kernel.h ensure_gelu_table)
        dev = next((b.device for b in self.buffers() if b.is_cuda), None)
        if dev is not None:
            from mixdq_amd import _C
            _C.gelu_table(dev)
            _C.silu_table(dev)              # ... and the SiLU table of the large GroupNorm apply launches (fused_norm.hip)
            if WEIGHT_ARENA:
                # every static tensor of the converted network in ONE allocation, in module order (arena.py)
                from mixdq_amd.arena import pack_static_
                self.__dict__["_arena"] = pack_static_(self, dev)
                self.__dict__.pop("_pf_plans", None)
        return self

    def set_fused(self, enabled: bool = True):
        """Switch the producer fusions on or off for the whole graph (see the top of this file)."""
        self.__dict__.pop("_pf_plans", None)
        for m in self.modules():
            if hasattr(type(m), "fused"):
                m.fused = bool(enabled)
            if isinstance(m, FeedForward):
                m.set_interleaved(bool(enabled))
        if enabled:
            self.prepare_fused_()
        return self

    # ---- the split conv_in of an inpainting checkpoint (cond_channels > 0) ---------------
    # conv_in(cat([x, c])) = conv(x; W[:, :4]) + conv(c; W[:, 4:]) + bias, and c -- the mask and the masked image's
    # latents -- is the same at every step of a run: the second term (with the bias) is computed once per run by
    # cond_term(), and a step's conv_in is the 4-channel conv with that term as the residual of its epilogue.
    def _conv_in_weight(self):
        w = getattr(self.conv_in, "weight", None)
        if w is None or getattr(self.conv_in, "valid_for_acceleration", False):
            raise RuntimeError("SDXLUNet: the split conv_in needs conv_in as a floating-point layer (a 9-channel "
                               "conv_in always is one: QuantizedConv2d falls back where in_channels % 4 != 0)")
        return w

    def _conv_in_split(self, refresh: bool):
        """(Wx8, Wc8): conv_in.weight[:, :out_channels] and [:, out_channels:], each zero-padded to 8 input channels,
        KRSC in memory: derived from conv_in.weight with `refresh`; without it (inside a captured step) only read."""
        if refresh:
            return derived.derive(derived.holder_of(self), "cin_split", (self._conv_in_weight(),),
                                  functools.partial(_split_pad8, self.cfg["out_channels"]),
                                  extra=self.cfg["out_channels"])
        out = derived.stored(self.__dict__.get("_derived_tensors"), "cin_split")
        if out is None:
            raise RuntimeError("SDXLUNet.forward: cond_term= should be what this UNet's cond_term() returned")
        return out

    @staticmethod
    def _pad8(x):
        """x [N, C <= 8, h, w] with zero channels up to 8, channels-last."""
        if x.shape[1] == 8:
            return x.contiguous(memory_format=torch.channels_last)
        xp = torch.zeros((x.shape[0], 8, x.shape[2], x.shape[3]), dtype=x.dtype, device=x.device
                         ).contiguous(memory_format=torch.channels_last)
        xp[:, :x.shape[1]] = x
        return xp

    def _conv_in_with_term(self, x, term):
        """conv_in of a step: conv(x8; Wx8) with `term` as the residual -- f16(f32(f16(sum)) + f32(T)), a torch half
        add of the two rounded tensors."""
        wx, _ = self._conv_in_split(refresh=False)
        x8 = self._pad8(x)
        if x8.is_cuda and x8.dtype == torch.float16:
            from mixdq_amd import _C
            return _C.conv2d_f16(x8, wx, None, 1, 1, _residual=term)
        return F.conv2d(x8, wx, None, 1, 1) + term

    def _apply(self, fn, recurse=True):          # .to() / .cuda() / .half(): the weights move, the plans go
        self.__dict__.pop("_pf_plans", None)
        # (... and the split conv_in weights: cond_term() / a ControlNet's hint_term() make them anew)
        derived.drop(self.__dict__.get("_derived_tensors"))
        return super()._apply(fn, recurse)

    def load_state_dict(self, *args, **kwargs):
        self.__dict__.pop("_pf_plans", None)
        return super().load_state_dict(*args, **kwargs)

    def _embed(self, sample, timestep, added_cond_kwargs):
        """The time embedding of a forward, with the addition embedding where the config has one: [B, time_embed_dim]."""
        cfg = self.cfg
        B = sample.shape[0]
        dtype = sample.dtype
        t = timestep
        if not torch.is_tensor(t):
            t = torch.tensor([t], dtype=torch.float32, device=sample.device)
        t = t.reshape(-1).expand(B)
        emb = self.time_embedding(sinusoidal_embedding(t, cfg["block_out_channels"][0]).to(dtype))
        if cfg.get("addition_embed_type", "text_time") is not None:    # (else: added_cond_kwargs is ignored)
            time_ids = added_cond_kwargs["time_ids"]
            text_embeds = added_cond_kwargs["text_embeds"]
            tid = sinusoidal_embedding(time_ids.flatten(), cfg["addition_time_embed_dim"])
            add = torch.cat([text_embeds, tid.reshape(B, -1).to(dtype)], dim=-1)
            emb = emb + self.add_embedding(add)
        return emb

    def _with_prefetch(self, sample, body):
        """body() -- the blocks of a forward -- under this network's weight-prefetch plan, where one applies."""
        use_pf = bool(self.fused and PREFETCH and sample.is_cuda and _fusable_f16(sample) and not DEFUSE)
        if not use_pf:
            return body()
        # Trace this forward's weight order and replay the plan of the last forward ON THIS DEVICE: the state
        # is this call's own PrefetchContext (thread-local while it runs), the plans are kept per device in
        # the instance and hold weak references -- a plan made for another device, or for weights that have
        # been replaced since (`.to()`, re-quantization, load_state_dict: cleared in _apply / below, and
        # dropped here when a reference is dead or points elsewhere), is never handed to a launch.
        from mixdq_amd import _C
        plans = self.__dict__.setdefault("_pf_plans", {})
        plan = plans.get(sample.device)
        if plan is not None and not _plan_alive(plan, sample.device):
            plans.pop(sample.device, None)
            plan = None
        ctx = _C.PrefetchContext(sample.device, plan["lists"] if plan else None)
        try:
            with ctx:
                return body()
        finally:
            if ctx._outer is None:                               # (an inner, inactive context traced nothing)
                sig = _trace_signature(ctx.trace)
                if plan is None or plan["sig"] != sig:           # first forward here, or the layers changed
                    new = _build_prefetch_plan(ctx.trace)
                    if new is None:
                        plans.pop(sample.device, None)
                    else:
                        plans[sample.device] = new


class SDXLUNet(FusedGraph):
    """forward(sample, timestep, encoder_hidden_states, added_cond_kwargs, return_dict=False)
    -> (noise_pred,), the call shape of quantize_sdxl.py:375-385.  `cfg`: overrides of SDXL_CONFIG; SD15_CONFIG
    makes it the SD 1.5 UNet (same classes, diffusers' names for that network)."""

    def __init__(self, cfg=None):
        super().__init__()
        cfg = dict(SDXL_CONFIG, **(cfg or {}))
        self.cfg = cfg
        boc = cfg["block_out_channels"]
        temb = cfg["time_embed_dim"]
        self.conv_in = nn.Conv2d(cfg["in_channels"], boc[0], 3, 1, 1)
        # input channels beyond the latents': 0, or the 5 (mask + masked-image latents) of an inpainting checkpoint
        self.cond_channels = cfg["in_channels"] - cfg["out_channels"]
        self.time_embedding = TimestepEmbedding(boc[0], temb)
        if cfg.get("addition_embed_type", "text_time") is not None:
            self.add_embedding = TimestepEmbedding(cfg["projection_class_embeddings_input_dim"], temb)
        n = cfg["layers_per_block"]
        depths = cfg["transformer_layers_per_block"]
        self.down_blocks = nn.ModuleList()
        skip = [boc[0]]
        cin = boc[0]
        for i, cout in enumerate(boc):
            last = i == len(boc) - 1
            self.down_blocks.append(DownBlock(cin, cout, temb, n, depths[i], cfg, not last))
            skip += [cout] * n + ([] if last else [cout])
            cin = cout
        self.mid_block = MidBlock(boc[-1], temb, cfg["mid_transformer_layers"], cfg)
        self.up_blocks = nn.ModuleList()
        prev = boc[-1]
        for i, cout in enumerate(reversed(boc)):
            last = i == len(boc) - 1
            sk = [skip.pop() for _ in range(n + 1)]
            self.up_blocks.append(UpBlock(prev, cout, sk, temb, list(reversed(depths))[i], cfg,
                                          not last))
            prev = cout
        self.conv_norm_out = nn.GroupNorm(cfg["norm_num_groups"], boc[0], eps=1e-5)
        self.conv_act = nn.SiLU()          # (diffusers' name)
        self.conv_out = nn.Conv2d(boc[0], cfg["out_channels"], 3, 1, 1)
        self.register_load_state_dict_post_hook(derived.after_load)

    @torch.no_grad()
    def cond_term(self, cond):
        """The part of conv_in's output that the conditioning channels contribute, bias included: cond [N, Cc, h, w]
        (Cc = cond_channels: for an inpainting checkpoint the latent-resolution mask, then the latents of the image
        with the masked pixels blanked) or the padded 8-channel form _C.inpaint_cond writes, in conv_in's dtype (FP16
        on the GPU) -> T = conv2d_f16(cond8, Wc8, bias=conv_in.bias, 1, 1), channels-last [N, C0, h, w].  The padding
        columns of Wc8 are zero, so what the padding channels of an 8-channel `cond` hold is irrelevant as long as it
        is finite.  Pass it as forward(sample4, ..., cond_term=T) at every step of the run.  The split weights are
        re-derived here, in place, when conv_in.weight was replaced or written since: call it after a reload, outside
        a captured graph (Sampler.sample does, at every call)."""
        if self.cond_channels <= 0:
            raise RuntimeError("SDXLUNet.cond_term: this UNet has no conditioning channels (in_channels == "
                               "out_channels)")
        if self.cond_channels > 8:
            raise RuntimeError("SDXLUNet.cond_term: at most 8 conditioning channels")
        w = self._conv_in_weight()
        if not (torch.is_tensor(cond) and cond.dim() == 4 and cond.shape[1] in (self.cond_channels, 8)
                and cond.dtype == w.dtype and cond.device == w.device):
            raise RuntimeError(f"SDXLUNet.cond_term: cond should be a [N, {self.cond_channels} or 8, h, w] {w.dtype} "
                               f"tensor on {w.device}")
        _, wc = self._conv_in_split(refresh=True)
        c8 = self._pad8(cond)
        bias = self.conv_in.bias
        if c8.is_cuda and c8.dtype == torch.float16:
            from mixdq_amd import _C
            return _C.conv2d_f16(c8, wc, bias, 1, 1)
        return F.conv2d(c8, wc, bias, 1, 1).contiguous(memory_format=torch.channels_last)

    def _check_cond_term(self, sample, cond_term):
        co, cc = self.cfg["out_channels"], self.cond_channels
        if cond_term is None:
            if cc > 0 and sample.shape[1] == co:
                raise RuntimeError(f"SDXLUNet.forward: this UNet has {cc} conditioning channels: a {co}-channel sample "
                                   f"needs cond_term= (unet.cond_term(cond)), or pass all {co + cc} channels")
            return
        if cc <= 0:
            raise RuntimeError("SDXLUNet.forward: cond_term given, but this UNet has no conditioning channels")
        if sample.dim() != 4 or sample.shape[1] != co:
            raise RuntimeError(f"SDXLUNet.forward: with cond_term the sample should have {co} channels")
        want = (sample.shape[0], self.conv_in.out_channels, sample.shape[2], sample.shape[3])
        if not (torch.is_tensor(cond_term) and tuple(cond_term.shape) == want and cond_term.dtype == sample.dtype
                and cond_term.device == sample.device
                and cond_term.is_contiguous(memory_format=torch.channels_last)):
            raise RuntimeError(f"SDXLUNet.forward: cond_term should be a channels-last {sample.dtype} tensor of shape "
                               f"{want} (one row per sample row) on the sample's device")

    def forward(self, sample, timestep, encoder_hidden_states, added_cond_kwargs=None,
                return_dict=False, cond_term=None, down_block_additional_residuals=None,
                mid_block_additional_residual=None, control=None):
        """`cond_term` (UNets with cond_channels > 0): what cond_term(cond) returned, one row per row of `sample`,
        which then has out_channels channels -- conv_in runs split, without a concatenated input.  Without it such a
        UNet takes all in_channels channels in `sample` (the drop-in form).

        `down_block_additional_residuals` / `mid_block_additional_residual`: diffusers' keywords and meaning -- a
        ControlNet's outputs ALREADY scaled, one tensor per skip (conv_in's output first) and one for the mid-block
        output; every skip becomes skip + r and the mid-block output x + r, in the sample's dtype.
        `control`: a ControlResiduals (unscaled residuals of 1 to 4 nets, a device table of per-step scales and the
        device step counter): what a device-side sampling loop passes instead.  One or the other."""
        self._check_cond_term(sample, cond_term)
        control = self._control_of(sample, down_block_additional_residuals, mid_block_additional_residual, control)
        emb = self._embed(sample, timestep, added_cond_kwargs)
        return self._with_prefetch(sample, lambda: self._forward_body(sample, emb, encoder_hidden_states, cond_term,
                                                                      control))

    # ---- ControlNet residuals ------------------------------------------------------------
    def n_skips(self) -> int:
        """How many skip tensors the down path makes (conv_in's output included): a ControlNet has one residual each."""
        return 1 + sum(len(b.resnets) + (1 if b.has_down else 0) for b in self.down_blocks)

    def _control_of(self, sample, down, mid, control):
        """The ControlResiduals of a forward: `control` itself, the diffusers keywords as one net with the scale table
        [[1.0]] at step 0 (f16(r * 1.0) is r: exactly skip + r), or None.  Counts and types are checked here, shapes
        where the skips exist (_add_control)."""
        if control is None and down is None and mid is None:
            return None
        if control is not None:
            if down is not None or mid is not None:
                raise RuntimeError("SDXLUNet.forward: control= and down_block_additional_residuals / "
                                   "mid_block_additional_residual exclude each other")
            if not isinstance(control, ControlResiduals):
                raise RuntimeError("SDXLUNet.forward: control should be a mixdq_amd.unet.ControlResiduals")
        else:
            if down is None or mid is None:
                raise RuntimeError("SDXLUNet.forward: down_block_additional_residuals and mid_block_additional_residual "
                                   "go together")
            if not isinstance(down, (list, tuple)):
                raise RuntimeError("SDXLUNet.forward: down_block_additional_residuals should be a list or tuple of "
                                   "tensors")
            control = ControlResiduals([(down, mid)], *_unit_scale(sample.device))
        n = self.n_skips()
        if not 1 <= len(control.nets) <= 4:
            raise RuntimeError(f"SDXLUNet.forward: 1 to 4 ControlNets, got {len(control.nets)}")
        for k, (d, m) in enumerate(control.nets):
            if len(d) != n:
                raise RuntimeError(f"SDXLUNet.forward: this UNet has {n} skip tensors: net {k} should bring {n} down "
                                   f"residuals, got {len(d)}")
            if not (torch.is_tensor(m) and all(torch.is_tensor(r) for r in d)):
                raise RuntimeError(f"SDXLUNet.forward: the residuals of net {k} should be tensors")
        sc, st = control.scales, control.step
        if not (torch.is_tensor(sc) and sc.dtype == torch.float32 and sc.dim() == 2 and sc.shape[0] == len(control.nets)
                and sc.shape[1] >= 1 and sc.device == sample.device and sc.is_contiguous()):
            raise RuntimeError(f"SDXLUNet.forward: control.scales should be a contiguous fp32 [{len(control.nets)}, "
                               f"n_steps] tensor on the sample's device")
        if not (torch.is_tensor(st) and st.dtype == torch.int32 and st.numel() == 1 and st.device == sample.device):
            raise RuntimeError("SDXLUNet.forward: control.step should be one int32 on the sample's device")
        return control

    def _add_control(self, skips, x, control):
        """(skips + residuals, x + mid residual) as FRESH tensors: a skip is also the next block's input and may carry
        a handed-off INT8 operand, so nothing is written in place.  Fused: ONE control_add launch over all of them;
        de-fused, on the CPU, for other dtypes or with MIXDQ_CONTROL_ADD=0: torch operations in the same order."""
        segs = list(skips) + [x]
        nets = [list(d) + [m] for d, m in control.nets]
        for k, net in enumerate(nets):
            for i, (s, r) in enumerate(zip(segs, net)):
                name = f"net {k}, " + (f"down residual {i}" if i < len(skips) else "the mid residual")
                if not (tuple(r.shape) == tuple(s.shape) and r.dtype == s.dtype and r.device == s.device
                        and r.is_contiguous(memory_format=torch.channels_last)):
                    raise RuntimeError(f"SDXLUNet.forward: {name} should be a channels-last {s.dtype} tensor of shape "
                                       f"{tuple(s.shape)} on the sample's device, got {tuple(r.shape)} {r.dtype}")
        segs = [s.contiguous(memory_format=torch.channels_last) for s in segs]
        if self.fused and not DEFUSE and CONTROL_ADD and all(_fusable_f16(s) for s in segs):
            from mixdq_amd import _C
            out = _C.control_add(segs, nets, control.scales, control.step)
        else:
            out = _control_add_torch(segs, nets, control.scales, control.step)
        return out[:-1], out[-1]

    def _forward_body(self, sample, emb, encoder_hidden_states, cond_term=None, control=None):
        if self.fused and _fusable_f16(sample) and not DEFUSE:
            self._project_temb_ahead(emb)
            self._project_context_ahead(encoder_hidden_states)
        x = sample.contiguous(memory_format=torch.channels_last)
        x = self.conv_in(x) if cond_term is None else self._conv_in_with_term(x, cond_term)
        skips = [x]
        for blk in self.down_blocks:
            x, outs = blk(x, emb, encoder_hidden_states)
            skips += outs
        x = self.mid_block(x, emb, encoder_hidden_states)
        if control is not None:
            skips, x = self._add_control(skips, x, control)
        for blk in self.up_blocks:
            x = blk(x, skips, emb, encoder_hidden_states)
        if self.fused and _fusable_f16(x):
            feed, q = _gn_feed(self.conv_norm_out, x, self.conv_out, silu=True)
            x = self.conv_out.forward_quantized(feed) if q else self.conv_out(feed)
        else:
            x = self.conv_out(self.conv_act(self.conv_norm_out(x)))
        return (x,)


_UNIT_SCALE = {}


def _unit_scale(device):
    """The scale table [[1.0]] and the step 0 of the keyword form, constants of the device: made once, so that the
    keyword form is the one control_add launch (never cached while a stream is capturing: a tensor that only a graph
    replay fills must not outlive the capture)."""
    got = _UNIT_SCALE.get(device)
    if got is None:
        got = (torch.ones((1, 1), dtype=torch.float32, device=device), torch.zeros(1, dtype=torch.int32, device=device))
        if not (device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            _UNIT_SCALE[device] = got
    return got


def _control_add_torch(segs, nets, scales, step):
    """control_add's arithmetic as torch operations in the segments' dtype: per net r * c_k (the python float of the
    fp32 scale), the nets summed left to right, then skip + sum; a net whose scale is 0, and every net at a step
    outside the table, is skipped; nothing added: a copy.  Reads the scales on the host (a synchronisation)."""
    st = int(step.item())
    row = [float(v) for v in scales[:, st].tolist()] if 0 <= st < scales.shape[1] else [0.0] * len(nets)
    out = []
    for i, s in enumerate(segs):
        acc = None
        for k, net in enumerate(nets):
            if row[k] == 0.0:
                continue
            t = net[i] * row[k]
            acc = t if acc is None else acc + t
        out.append(s.clone() if acc is None else s + acc)
    return out


# ---------------------------------------------------------------------------------------------
# synthetic weights, layer inventory
# ---------------------------------------------------------------------------------------------
def quantizable_layers(unet: nn.Module) -> "OrderedDict[str, nn.Module]":
    """name -> nn.Linear / nn.Conv2d in named_modules() order: the keys of the bit-width yamls."""
    return OrderedDict((n, m) for n, m in unet.named_modules()
                       if isinstance(m, (nn.Linear, nn.Conv2d)))


@torch.no_grad()
def init_synthetic_weights(unet: nn.Module, seed: int = 42, std: float = 0.02):
    """randn * 0.02, generator seeded with seed + layer index."""
    for idx, (name, mod) in enumerate(quantizable_layers(unet).items()):
        g = torch.Generator(device="cpu").manual_seed(seed + idx)
        mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * std)
        if mod.bias is not None:
            mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * std)
    return unet


def build_unet(device=None, dtype=torch.float16, seed: int = 42, cfg=None) -> SDXLUNet:
    unet = SDXLUNet(cfg)
    init_synthetic_weights(unet, seed)
    unet = unet.to(dtype=dtype)
    if device is not None:
        unet = unet.to(device)
    unet = unet.to(memory_format=torch.channels_last)
    return unet.eval()
