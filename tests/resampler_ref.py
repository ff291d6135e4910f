"""The perceiver Resampler of the IP-Adapter "plus" checkpoints from stock torch functions, driven by a state dict with
the checkpoint's `image_proj.*` names: the network mixdq_amd.ip_adapter.Resampler is compared with (in FP32 on the CPU
as the truth, in FP16 on the GPU as the yardstick of what FP16 costs)."""
import torch
import torch.nn.functional as F


def forward(sd, hidden, heads, depth, eps=1e-5):
    """sd: the Resampler's state dict in the dtype and on the device of `hidden` [B, n1, embedding_dim]."""
    def ln(x, name):
        return F.layer_norm(x, x.shape[-1:], sd[name + ".weight"], sd[name + ".bias"], eps)

    x = F.linear(hidden, sd["proj_in.weight"], sd["proj_in.bias"])
    B = hidden.shape[0]
    lat = sd["latents"].repeat(B, 1, 1)
    for i in range(depth):
        a = f"layers.{i}.0."
        xn, latn = ln(x, a + "norm1"), ln(lat, a + "norm2")
        q = F.linear(latn, sd[a + "to_q.weight"])
        k, v = F.linear(torch.cat([xn, latn], dim=1), sd[a + "to_kv.weight"]).chunk(2, dim=-1)
        q, k, v = (t.reshape(B, t.shape[1], heads, -1).transpose(1, 2) for t in (q, k, v))
        w = torch.softmax((q @ k.transpose(-1, -2)).float() * q.shape[-1] ** -0.5, dim=-1).to(v.dtype)
        lat = lat + F.linear((w @ v).transpose(1, 2).reshape(B, lat.shape[1], -1), sd[a + "to_out.weight"])
        f = f"layers.{i}.1."
        lat = lat + F.linear(F.gelu(F.linear(ln(lat, f + "0"), sd[f + "1.weight"])), sd[f + "3.weight"])
    return ln(F.linear(lat, sd["proj_out.weight"], sd["proj_out.bias"]), "norm_out")
