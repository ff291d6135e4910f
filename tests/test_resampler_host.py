"""The Resampler of the IP-Adapter "plus" checkpoints on the CPU: parameter names and counts, the plain forward against
the stock network, the norm1-folded to_kv weight, what `tokens` refuses, and the argument checks of the two new entry
points that return before any HIP call.  No GPU."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from mixdq_amd.ip_adapter import RESAMPLER_PLUS_SD15, RESAMPLER_PLUS_SDXL, Resampler, build_ip_adapter
from mixdq_amd.unet import SD15_CONFIG, SDXL_CONFIG
from tests import resampler_ref
from tests.test_ip_adapter_host import TINY

SMALL = dict(dim=128, depth=2, dim_head=64, heads=2, embedding_dim=96, ff_mult=2)


@pytest.mark.parametrize("unet,cfg,cross,count", [(SD15_CONFIG, RESAMPLER_PLUS_SD15, 768, 29918208),
                                                  (SDXL_CONFIG, RESAMPLER_PLUS_SDXL, 2048, None)], ids=["sd15", "sdxl"])
def test_state_dict_names_and_parameter_count(unet, cfg, cross, count):
    ad = build_ip_adapter(unet, 1024, num_tokens=16, resampler=cfg, device="meta")
    sd = {k[len("image_proj."):]: v for k, v in ad.state_dict().items() if k.startswith("image_proj.")}
    dim, inner, hid, emb = cfg["dim"], cfg["dim_head"] * cfg["heads"], cfg["dim"] * cfg["ff_mult"], cfg["embedding_dim"]
    want = {"latents": (1, 16, dim), "proj_in.weight": (dim, emb), "proj_in.bias": (dim,), "proj_out.weight": (cross, dim),
            "proj_out.bias": (cross,), "norm_out.weight": (cross,), "norm_out.bias": (cross,)}
    for i in range(cfg["depth"]):
        for n in ("norm1", "norm2"):
            want[f"layers.{i}.0.{n}.weight"] = want[f"layers.{i}.0.{n}.bias"] = (dim,)
        want[f"layers.{i}.0.to_q.weight"], want[f"layers.{i}.0.to_kv.weight"] = (inner, dim), (2 * inner, dim)
        want[f"layers.{i}.0.to_out.weight"] = (dim, inner)
        want[f"layers.{i}.1.0.weight"] = want[f"layers.{i}.1.0.bias"] = (dim,)
        want[f"layers.{i}.1.1.weight"], want[f"layers.{i}.1.3.weight"] = (hid, dim), (dim, hid)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    total = sum(v.numel() for v in sd.values())
    # by the shapes: 7 dim + T dim + dim emb + cross dim + 3 cross + depth (6 dim + 4 inner dim + 2 dim hid)
    by_shape = (16 + 1) * dim + dim * emb + cross * dim + 3 * cross + cfg["depth"] * (6 * dim + 4 * inner * dim + 2 * dim * hid)
    assert total == by_shape and (count is None or total == count)


@pytest.mark.parametrize("T,n1,B", [(5, 10, 1), (16, 50, 2)])
def test_cpu_forward_is_the_stock_network(T, n1, B):
    rs = Resampler(num_queries=T, output_dim=64, **SMALL).eval()
    hidden = torch.randn(B, n1, 96, generator=torch.Generator().manual_seed(T))
    want = resampler_ref.forward(rs.state_dict(), hidden, heads=2, depth=2)
    torch.testing.assert_close(rs(hidden), want, rtol=1e-5, atol=1e-5)


def test_folded_weight_reproduces_to_kv_of_norm1():
    rs = Resampler(num_queries=4, output_dim=64, **SMALL).double().eval()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for attn, _ in rs.layers:
            attn.norm1.weight.copy_(1 + 0.3 * torch.randn(128, generator=g, dtype=torch.float64))
            attn.norm1.bias.copy_(0.3 * torch.randn(128, generator=g, dtype=torch.float64))
    x = torch.randn(2, 7, 128, generator=g, dtype=torch.float64) * 3 + 1
    w, b = rs.folded_kv()
    got = F.linear(F.layer_norm(x, (128,)), w, b)
    for i, (attn, _) in enumerate(rs.layers):
        want = attn.to_kv(attn.norm1(x))
        assert (got[..., 256 * i:256 * (i + 1)] - want).abs().max().item() <= 1e-12


def test_tokens_refuses_the_other_adapters_input():
    plus = build_ip_adapter(TINY, 24, num_tokens=4, resampler=dict(SMALL, depth=1), dtype=torch.float32)
    plain = build_ip_adapter(TINY, 24, num_tokens=4, dtype=torch.float32)
    assert tuple(plus.tokens(torch.zeros(2, 9, 96)).shape) == (2, 4, 48)
    with pytest.raises(RuntimeError, match="has a Resampler"):
        plus.tokens(torch.zeros(2, 96))
    with pytest.raises(RuntimeError, match="has no Resampler"):
        plain.tokens(torch.zeros(2, 9, 24))


def test_entry_points_validate_before_any_hip_call():
    from mixdq_amd.build import build
    lib = ctypes.CDLL(build())
    vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    INVALID, ALIGN, UNSUPPORTED, SHAPE = 1, 2, 3, 9
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 63) & ~63                       # host memory: never dereferenced by these calls

    att = lib.mixdq_attention_f16_perceiver
    att.argtypes, att.restype = [vp] * 6 + [i32] * 6 + [i64] * 12 + [f32, vp], i32

    def attn(q=p, k1=p, v1=p, k2=p, v2=p, out=p, batch=1, heads=1, hd=64, tq=16, t1=8, t2=8, strides=(1024, 64) * 6):
        return att(q, k1, v1, k2, v2, out, batch, heads, hd, tq, t1, t2, *strides, 0.125, None)
    assert attn(tq=17) == SHAPE and attn(tq=0) == SHAPE and attn(hd=80) == SHAPE and attn(t1=0) == SHAPE
    assert attn(t2=-1) == SHAPE and attn(t1=4090, t2=7) == SHAPE
    assert attn(q=None) == INVALID and attn(k2=None) == INVALID and attn(heads=0) == INVALID and attn(batch=-1) == INVALID
    assert attn(strides=(1024, 64) * 5 + (1024, 68)) == ALIGN and attn(v1=p + 8) == ALIGN
    assert attn(batch=0) == 0 and attn(batch=0, k2=None, v2=None, t2=0) == 0

    lin = lib.mixdq_linear_f16_skinny
    lin.argtypes, lin.restype = [vp, i64, vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, f32, i32, vp], i32

    def skinny(A=p, lda=None, W=p, bias=None, res=None, D=p + 2048, ldd=None, M=1, N=16, K=32, lw=None, lb=None, flags=0):
        return lin(A, K if lda is None else lda, W, bias, res, D, N if ldd is None else ldd, M, N, K, lw, lb, 1e-5, flags, None)
    assert skinny(N=24) == SHAPE and skinny(K=48) == SHAPE and skinny(M=257) == SHAPE and skinny(M=0) == SHAPE
    assert skinny(K=8224) == SHAPE and skinny(K=4096, lw=p, lb=p) == SHAPE and skinny(lda=16) == SHAPE
    assert skinny(lw=p) == INVALID and skinny(lb=p) == INVALID and skinny(A=None) == INVALID
    assert skinny(D=p) == INVALID and skinny(res=p + 2048 + 8) == INVALID       # D on A; a residual half on D
    assert skinny(lda=36) == ALIGN and skinny(bias=p + 4) == ALIGN and skinny(flags=128) == UNSUPPORTED
