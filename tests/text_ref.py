"""The text encoder of mixdq_amd.text restated with stock torch modules (nn.Embedding / nn.LayerNorm / nn.Linear /
scaled_dot_product_attention(is_causal=True)), any dtype and device: transformers' CLIPTextModel[WithProjection]
layer by layer.  Takes the state dict of a mixdq_amd.text.TextEncoder (transformers' names)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


class _Attn(nn.Module):
    def __init__(self, c, heads):
        super().__init__()
        self.heads = heads
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = (nn.Linear(c, c) for _ in range(4))

    def forward(self, x):
        B, T, C = x.shape
        q, k, v = (f(x).view(B, T, self.heads, C // self.heads).transpose(1, 2)
                   for f in (self.q_proj, self.k_proj, self.v_proj))
        o = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        return self.out_proj(o.transpose(1, 2).reshape(B, T, C))


class _MLP(nn.Module):
    def __init__(self, c, inter, act):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(c, inter), nn.Linear(inter, c)
        self.act = quick_gelu if act == "quick_gelu" else F.gelu

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


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


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.token_embedding = nn.Embedding(cfg["vocab_size"], cfg["hidden_size"])
        self.position_embedding = nn.Embedding(cfg["max_position_embeddings"], cfg["hidden_size"])


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(cfg) for _ in range(cfg["num_hidden_layers"])])


class _Transformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings, self.encoder = _Embeddings(cfg), _Encoder(cfg)
        self.final_layer_norm = nn.LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])


class StockTextEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.text_model = _Transformer(cfg)
        if cfg.get("projection_dim"):
            self.text_projection = nn.Linear(cfg["hidden_size"], cfg["projection_dim"], bias=False)

    @torch.no_grad()
    def forward(self, ids):
        """(last_hidden_state, penultimate, pooled)"""
        tm = self.text_model
        B, T = ids.shape
        x = tm.embeddings.token_embedding(ids) + tm.embeddings.position_embedding(torch.arange(T, device=ids.device))
        pen = x
        for layer in tm.encoder.layers:
            pen = x
            x = layer(x)
        last = tm.final_layer_norm(x)
        pooled = last[torch.arange(B, device=ids.device), ids.argmax(-1)]
        if hasattr(self, "text_projection"):
            pooled = self.text_projection(pooled)
        return last, pen, pooled


def stock_encoder(cfg, state_dict, dtype, device):
    """The stock network with `state_dict`'s weights (FP16 values, upcast exactly when dtype is wider)."""
    m = StockTextEncoder(cfg)
    m.load_state_dict({k: v.detach().to("cpu", torch.float32) for k, v in state_dict.items()}, strict=True)
    return m.to(device=device, dtype=dtype).eval()
