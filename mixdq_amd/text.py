"""The FP16 CLIP text encoders (transformers' CLIPTextModel / CLIPTextModelWithProjection) on this library's kernels:
token ids in, the UNet's conditioning out.

    enc_l = build_text_encoder(CLIP_L_CONFIG, device="cuda")         # synthetic weights; load_state_dict takes
    enc_g = build_text_encoder(OPENCLIP_BIGG_CONFIG, device="cuda")  # transformers' names
    encoder_hidden_states, text_embeds = encode_sdxl(enc_l, enc_g, ids_l, ids_g)     # [B, 77, 2048], [B, 1280]

Every layer runs in FP16 on the C-ABI library: mixdq_embed_tokens_f16 (token + position gather), per layer
mixdq_layernorm_quantize with its FP16 output (n_out = 0), ONE q|k|v mixdq_linear_f16 (N = 3C), mixdq_attention_f16 on
the three column slices with MIXDQ_FLAG_CAUSAL (77 tokens, 64-wide heads: the short-key kernel), out_proj with the
layer input as residual, LayerNorm, fc1 with the activation in its epilogue (MIXDQ_FLAG_ACT_GELU / _QUICK_GELU) and
fc2 with the residual.  The only torch operators of a forward are the id dtype conversion, the argmax / row gather of
the pooled output and views (encode_sdxl adds one torch.cat); none waits for the GPU, so `hip_graph_opt(encoder)`
captures it.

There is no tokenizer here (the interface takes token ids, as CLIPTextModel does), no attention-mask / padding-mask
input (CLIP's text tower is run with the causal mask alone), and FP16 only.  A floating-point path with no counterpart
in the reference (which reaches the encoders through diffusers' pipeline): held to tolerance against the same network
built from stock torch modules (tests/text_ref.py).  DESIGN.md section 3.24.
"""
from collections import OrderedDict, namedtuple

import torch
import torch.nn as nn

from mixdq_amd.derived import DerivedWeights

CLIP_L_CONFIG = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                     hidden_act="quick_gelu", projection_dim=None, vocab_size=49408, max_position_embeddings=77,
                     layer_norm_eps=1e-5)
OPENCLIP_BIGG_CONFIG = dict(hidden_size=1280, num_hidden_layers=32, num_attention_heads=20, intermediate_size=5120,
                            hidden_act="gelu", projection_dim=1280, vocab_size=49408, max_position_embeddings=77,
                            layer_norm_eps=1e-5)
# SD 2.x's encoder: OpenCLIP ViT-H/14's text tower (hidden 1024, 16 heads, intermediate 4096, GELU).  The tower has 24
# layers and SD 2.x conditions on final_layer_norm of the PENULTIMATE one's output; the checkpoints ship that as a
# CLIPTextModel without the last layer (num_hidden_layers 23), so `last_hidden_state` -- encode_sd15 -- is the
# conditioning [B, T, 1024] mixdq_amd.unet.SD21_CONFIG reads.  Configuration alone: no code knows about it.
OPENCLIP_H_CONFIG = dict(hidden_size=1024, num_hidden_layers=23, num_attention_heads=16, intermediate_size=4096,
                         hidden_act="gelu", projection_dim=None, vocab_size=49408, max_position_embeddings=77,
                         layer_norm_eps=1e-5)
HEAD_DIM = 64                   # every encoder here; the width MIXDQ_FLAG_CAUSAL is built for
ACTIVATIONS = ("gelu", "quick_gelu")

TextEncoderOutput = namedtuple("TextEncoderOutput", ["last_hidden_state", "penultimate", "pooled"])


class ClipEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.token_embedding = nn.Embedding(cfg["vocab_size"], cfg["hidden_size"])
        self.position_embedding = nn.Embedding(cfg["max_position_embeddings"], cfg["hidden_size"])


def _cat_qkv(_old, wq, bq, wk, bk, wv, bv):
    return torch.cat([wq, wk, wv]).contiguous(), torch.cat([bq, bk, bv]).contiguous()


class ClipAttention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)
        self.out_proj = nn.Linear(c, c)

    def qkv(self):
        """q_proj | k_proj | v_proj as ONE [3C, C] projection."""
        return _cat_qkv(None, *self.qkv_sources())

    def qkv_sources(self):
        return tuple(p for m in (self.q_proj, self.k_proj, self.v_proj) for p in (m.weight, m.bias))


class ClipMLP(nn.Module):
    def __init__(self, c, inter):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(c, inter), nn.Linear(inter, c)


class ClipLayer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        c, eps = cfg["hidden_size"], cfg["layer_norm_eps"]
        self.layer_norm1 = nn.LayerNorm(c, eps=eps)
        self.self_attn = ClipAttention(c)
        self.layer_norm2 = nn.LayerNorm(c, eps=eps)
        self.mlp = ClipMLP(c, cfg["intermediate_size"])

    def run(self, enc, x, qkv):
        from mixdq_amd import _C
        C = x.shape[-1]
        h = enc._ln(self.layer_norm1, x)
        p = _C.linear_f16(h, *qkv)
        att = _C.attention_f16(p[..., :C], p[..., C:2 * C], p[..., 2 * C:], enc.heads, _causal=True)
        x = _C.linear_f16(att, self.self_attn.out_proj.weight, self.self_attn.out_proj.bias, _residual=x)
        h = _C.linear_f16(enc._ln(self.layer_norm2, x), self.mlp.fc1.weight, self.mlp.fc1.bias, _act=enc.act)
        return _C.linear_f16(h, self.mlp.fc2.weight, self.mlp.fc2.bias, _residual=x)


class ClipEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([ClipLayer(cfg) for _ in range(cfg["num_hidden_layers"])])


class ClipTextTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = ClipEmbeddings(cfg)
        self.encoder = ClipEncoder(cfg)
        self.final_layer_norm = nn.LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])


class TextEncoder(DerivedWeights, nn.Module):
    """A CLIPTextModel (projection_dim None) or CLIPTextModelWithProjection, parameter names as transformers'."""

    def __init__(self, cfg=None):
        super().__init__()
        self.cfg = dict(CLIP_L_CONFIG if cfg is None else cfg)
        c, heads = self.cfg["hidden_size"], self.cfg["num_attention_heads"]
        if c != heads * HEAD_DIM:
            raise ValueError("TextEncoder: hidden_size should be num_attention_heads x %d" % HEAD_DIM)
        if self.cfg["hidden_act"] not in ACTIVATIONS:
            raise ValueError("TextEncoder: hidden_act should be one of %r" % (ACTIVATIONS,))
        self.heads, self.act = heads, self.cfg["hidden_act"]
        self.text_model = ClipTextTransformer(self.cfg)
        if self.cfg.get("projection_dim"):
            self.text_projection = nn.Linear(c, self.cfg["projection_dim"], bias=False)
        self._init_derived()

    def _derive(self):
        """The derived weights (lifecycle: DerivedWeights): layer index -> its q|k|v projection."""
        return {i: (layer.self_attn.qkv_sources(), _cat_qkv) for i, layer in enumerate(self.text_model.encoder.layers)}

    @staticmethod
    def _ln(norm, x):
        from mixdq_amd import _C
        return _C.layernorm_quantize(x, norm.weight, norm.bias, norm.eps, [], want_f16=True)[1]

    # ---- forward --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, ids):
        """ids [B, T] (int32 or int64, on the GPU, 1 <= T <= 77) -> TextEncoderOutput of FP16 tensors:
        last_hidden_state [B, T, C] (after final_layer_norm), penultimate [B, T, C] (the input of the last layer:
        transformers' hidden_states[-2], the one SDXL conditions on) and pooled [B, C or projection_dim] (the
        final_layer_norm row at ids.argmax(-1) -- the EOS position -- through text_projection where there is one).
        An id outside the vocabulary is clamped into it (see _C.embed_tokens_f16)."""
        from mixdq_amd import _C
        tmax = self.cfg["max_position_embeddings"]
        if not (torch.is_tensor(ids) and ids.is_cuda and ids.dim() == 2 and ids.dtype in (torch.int32, torch.int64)
                and 1 <= ids.shape[1] <= tmax):
            raise RuntimeError("TextEncoder.forward: ids should be a [B, T] int32 or int64 GPU tensor with 1 <= T <= %d"
                               % tmax)
        tm = self.text_model
        if any(p.dtype != torch.float16 for p in self.parameters()):          # (metadata only: no wait for the GPU)
            raise RuntimeError("TextEncoder.forward: the encoder runs in FP16 (build_text_encoder / .half())")
        B, C = ids.shape[0], self.cfg["hidden_size"]
        ids32 = ids.to(torch.int32).contiguous()
        qkv = self._derived()
        x = _C.embed_tokens_f16(ids32, tm.embeddings.token_embedding.weight, tm.embeddings.position_embedding.weight)
        penultimate = x
        for i, layer in enumerate(tm.encoder.layers):
            penultimate = x
            x = layer.run(self, x, qkv[i])
        last = self._ln(tm.final_layer_norm, x)
        eos = ids32.argmax(-1)                                           # the EOS token has the largest id
        pooled = last.gather(1, eos.view(B, 1, 1).expand(B, 1, C)).view(B, C)
        if hasattr(self, "text_projection"):
            pooled = _C.linear_f16(pooled, self.text_projection.weight, None)
        return TextEncoderOutput(last, penultimate, pooled)


def encode_sdxl(enc_l, enc_g, ids_l, ids_g):
    """SDXL's conditioning from its two encoders: (encoder_hidden_states [B, T, 768 + 1280] -- the two penultimate
    hidden states side by side -- and text_embeds [B, 1280], the projected pooled output of the second), as
    Sampler.sample / sample_image take them (added_cond_kwargs["text_embeds"])."""
    out_l, out_g = enc_l(ids_l), enc_g(ids_g)
    return torch.cat([out_l.penultimate, out_g.penultimate], dim=-1), out_g.pooled


def encode_sd15(enc_l, ids):
    """SD 1.5's conditioning: the last hidden state (after final_layer_norm) [B, T, 768]."""
    return enc_l(ids).last_hidden_state


def state_dict_names(cfg=None):
    """(name, shape) of every parameter of transformers' CLIPTextModel[WithProjection] with this config, written out
    from the layer list rather than read off the modules."""
    cfg = CLIP_L_CONFIG if cfg is None else cfg
    c, inter = cfg["hidden_size"], cfg["intermediate_size"]
    out = [("text_model.embeddings.token_embedding.weight", (cfg["vocab_size"], c)),
           ("text_model.embeddings.position_embedding.weight", (cfg["max_position_embeddings"], c))]
    lin = lambda n, o, i: [(n + ".weight", (o, i)), (n + ".bias", (o,))]
    norm = lambda n: [(n + ".weight", (c,)), (n + ".bias", (c,))]
    for i in range(cfg["num_hidden_layers"]):
        p = f"text_model.encoder.layers.{i}."
        for s in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out += lin(p + "self_attn." + s, c, c)
        out += norm(p + "layer_norm1")
        out += lin(p + "mlp.fc1", inter, c) + lin(p + "mlp.fc2", c, inter)
        out += norm(p + "layer_norm2")
    out += norm("text_model.final_layer_norm")
    if cfg.get("projection_dim"):
        out.append(("text_projection.weight", (cfg["projection_dim"], c)))
    return out


def parameter_count(cfg=None) -> int:
    n = 0
    for _, shape in state_dict_names(cfg):
        k = 1
        for d in shape:
            k *= d
        n += k
    return n


def build_text_encoder(cfg=None, seed: int = 42, device=None, dtype=torch.float16) -> TextEncoder:
    """An encoder with synthetic weights: randn * 0.02 per linear layer (init_synthetic_weights, as build_unet's) and
    per embedding table, LayerNorm weights 1 + randn * 0.1 and biases randn * 0.1; FP16, eval."""
    from mixdq_amd.unet import init_synthetic_weights
    enc = TextEncoder(cfg)
    with torch.no_grad():
        init_synthetic_weights(enc, seed)
        for idx, (name, mod) in enumerate(enc.named_modules()):
            g = torch.Generator(device="cpu").manual_seed(seed + 100003 + idx)
            if isinstance(mod, nn.Embedding):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * 0.02)
            elif isinstance(mod, nn.LayerNorm):
                mod.weight.copy_(1 + torch.randn(mod.weight.shape, generator=g) * 0.1)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
    enc = enc.to(dtype=dtype)
    if device is not None:
        enc = enc.to(device)
    return enc.eval()


def parameter_counts(enc) -> "OrderedDict[str, int]":
    """Parameters under `text_model.` and under `text_projection.`."""
    out = OrderedDict(text_model=0, text_projection=0)
    for n, p in enc.named_parameters():
        out[n.split(".")[0]] += p.numel()
    return out
