"""The VAE encoder of mixdq_amd.vae restated with stock torch modules (nn.Conv2d / nn.GroupNorm / F.pad /
scaled_dot_product_attention), NCHW, any dtype and device: diffusers' AutoencoderKL `quant_conv(encoder(x))` layer by
layer, on tests/vae_ref.py's ResNet and mid blocks.  Takes the state dict of a mixdq_amd.vae.VAEEncoder (diffusers'
names).

And the two ends of the encoder (mixdq_image_to_nhwc8_f16, mixdq_vae_latent_sample; arithmetic: include/mixdq_math.h)
restated in numpy float32: every operation one IEEE binary32 round-to-nearest ufunc call, in the specification's order,
the exponential from the oracle library's mixdq_oracle_expf."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.vae_ref import _Mid, _Res

f32 = np.float32


class _Downsampler(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, stride=2, padding=0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1)))


class _Down(nn.Module):
    def __init__(self, cin, cout, n, g, add_down):
        super().__init__()
        self.resnets = nn.ModuleList([_Res(cin if i == 0 else cout, cout, g) for i in range(n)])
        if add_down:
            self.downsamplers = nn.ModuleList([_Downsampler(cout)])

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        return self.downsamplers[0](x) if hasattr(self, "downsamplers") else x


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        ch, g = tuple(cfg["block_out_channels"]), cfg["norm_num_groups"]
        self.conv_in = nn.Conv2d(3, ch[0], 3, padding=1)
        self.down_blocks = nn.ModuleList([_Down(ch[max(i - 1, 0)], ch[i], cfg["layers_per_block"], g, i != len(ch) - 1)
                                          for i in range(len(ch))])
        self.mid_block = _Mid(ch[-1], g)
        self.conv_norm_out = nn.GroupNorm(g, ch[-1], eps=1e-6)
        self.conv_out = nn.Conv2d(ch[-1], 2 * cfg["latent_channels"], 3, padding=1)

    def forward(self, x):
        x = self.conv_in(x)
        for b in self.down_blocks:
            x = b(x)
        return self.conv_out(F.silu(self.conv_norm_out(self.mid_block(x))))


class StockVAEEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.encoder = _Encoder(cfg)
        self.quant_conv = nn.Conv2d(2 * cfg["latent_channels"], 2 * cfg["latent_channels"], 1)

    @torch.no_grad()
    def forward(self, image):
        """The moments [B, 2L, H/8, W/8]: mean | log-variance."""
        return self.quant_conv(self.encoder(image.to(self.quant_conv.weight.dtype)))


def stock_encoder(cfg, state_dict, dtype, device):
    """The stock network with `state_dict`'s weights (FP16 values, upcast exactly when dtype is wider)."""
    m = StockVAEEncoder(cfg)
    m.load_state_dict({k: v.detach().to("cpu", torch.float32) for k, v in state_dict.items()}, strict=True)
    return m.to(device=device, dtype=dtype).eval()


# ---- the ingest and the posterior sample, in numpy float32 -------------------------------------------------------
TWO_OVER_255 = np.array([0x3C008081], dtype=np.uint32).view(f32)[0]


def ingest(image):
    """image [B, C <= 8, H, W] uint8 / float16 / float32 (any strides) -> float16 [B, H, W, 8], channels C.. zero.
    uint8: f16(f32(u) * f32(2/255) - 1), the product and the difference rounded separately; floats: f16(f32(v))."""
    B, C, H, W = image.shape
    if image.dtype == np.uint8:
        v = image.astype(f32) * TWO_OVER_255
        v = v - f32(1.0)
    else:
        v = image.astype(f32)
    assert v.dtype == f32
    out = np.zeros((B, H, W, 8), dtype=np.float16)
    with np.errstate(over="ignore"):
        out[..., :C] = v.astype(np.float16).transpose(0, 2, 3, 1)
    return out


def latent_sample(oracle_lib, moments, noise, sf):
    """moments float16 [B, h, w, 2L] (mean | logvar), noise float32 [B, h, w, L] or None -> float32 [B, h, w, L]:
    lv = min(max(logvar, -30), 20); std = expf(0.5 * lv); z = (mean + std * noise) * sf; without noise mean * sf."""
    L = moments.shape[-1] // 2
    mean, sf = moments[..., :L].astype(f32), f32(sf)
    if noise is None:
        return mean * sf
    lv = np.minimum(np.maximum(moments[..., L:].astype(f32), f32(-30.0)), f32(20.0))
    half = f32(0.5) * lv
    std = np.array([oracle_lib.mixdq_oracle_expf(float(a)) for a in half.ravel()], f32).reshape(half.shape)
    z = (mean + std * noise.astype(f32)) * sf
    assert z.dtype == f32
    return z
