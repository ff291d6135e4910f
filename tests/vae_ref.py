"""The VAE decoder of mixdq_amd.vae restated with stock torch modules (nn.Conv2d / nn.GroupNorm / F.interpolate /
scaled_dot_product_attention), NCHW, any dtype and device: diffusers' AutoencoderKL.decode(z / scaling_factor) layer
by layer.  Takes the state dict of a mixdq_amd.vae.VAEDecoder (diffusers' names)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class _Res(nn.Module):
    def __init__(self, cin, cout, g):
        super().__init__()
        self.norm1, self.conv1 = nn.GroupNorm(g, cin, eps=1e-6), nn.Conv2d(cin, cout, 3, padding=1)
        self.norm2, self.conv2 = nn.GroupNorm(g, cout, eps=1e-6), nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.conv_shortcut = nn.Conv2d(cin, cout, 1)

    def forward(self, x):
        h = self.conv1(F.silu(self.norm1(x)))
        h = self.conv2(F.silu(self.norm2(h)))
        return (self.conv_shortcut(x) if hasattr(self, "conv_shortcut") else x) + h


class _Attn(nn.Module):
    def __init__(self, c, g):
        super().__init__()
        self.group_norm = nn.GroupNorm(g, c, eps=1e-6)
        self.to_q, self.to_k, self.to_v = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)
        self.to_out = nn.ModuleList([nn.Linear(c, c)])

    def forward(self, x):
        B, C, H, W = x.shape
        t = self.group_norm(x).view(B, C, H * W).transpose(1, 2)
        q, k, v = (f(t).unsqueeze(1) for f in (self.to_q, self.to_k, self.to_v))      # one head of width C
        o = F.scaled_dot_product_attention(q, k, v).squeeze(1)
        return x + self.to_out[0](o).transpose(1, 2).reshape(B, C, H, W)


class _Mid(nn.Module):
    def __init__(self, c, g):
        super().__init__()
        self.attentions = nn.ModuleList([_Attn(c, g)])
        self.resnets = nn.ModuleList([_Res(c, c, g), _Res(c, c, g)])

    def forward(self, x):
        return self.resnets[1](self.attentions[0](self.resnets[0](x)))


class _Upsampler(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, padding=1)

    def forward(self, x):
        return self.conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))


class _Up(nn.Module):
    def __init__(self, cin, cout, n, g, add_up):
        super().__init__()
        self.resnets = nn.ModuleList([_Res(cin if i == 0 else cout, cout, g) for i in range(n)])
        if add_up:
            self.upsamplers = nn.ModuleList([_Upsampler(cout)])

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        return self.upsamplers[0](x) if hasattr(self, "upsamplers") else x


class _Decoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        ch, g = tuple(cfg["block_out_channels"]), cfg["norm_num_groups"]
        rev = ch[::-1]
        self.conv_in = nn.Conv2d(cfg["latent_channels"], ch[-1], 3, padding=1)
        self.mid_block = _Mid(ch[-1], g)
        self.up_blocks = nn.ModuleList([_Up(rev[max(i - 1, 0)], rev[i], cfg["layers_per_block"] + 1, g, i != len(rev) - 1)
                                        for i in range(len(rev))])
        self.conv_norm_out = nn.GroupNorm(g, ch[0], eps=1e-6)
        self.conv_out = nn.Conv2d(ch[0], 3, 3, padding=1)

    def forward(self, x):
        x = self.mid_block(self.conv_in(x))
        for b in self.up_blocks:
            x = b(x)
        return self.conv_out(F.silu(self.conv_norm_out(x)))


class StockVAEDecoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.scaling_factor = cfg["scaling_factor"]
        self.post_quant_conv = nn.Conv2d(cfg["latent_channels"], cfg["latent_channels"], 1)
        self.decoder = _Decoder(cfg)

    @torch.no_grad()
    def forward(self, latents):
        z = latents.to(self.post_quant_conv.weight.dtype) / self.scaling_factor
        return self.decoder(self.post_quant_conv(z))


def stock_decoder(cfg, state_dict, dtype, device):
    """The stock network with `state_dict`'s weights (FP16 values, upcast exactly when dtype is wider)."""
    m = StockVAEDecoder(cfg)
    m.load_state_dict({k: v.detach().to("cpu", torch.float32) for k, v in state_dict.items()}, strict=True)
    return m.to(device=device, dtype=dtype).eval()
