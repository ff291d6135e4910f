"""GPU tests of the FP16 text encoders (mixdq_amd.text) on a small config that still reaches every kernel of the full
ones: the embedding gather, LayerNorm with FP16 output, the fused q|k|v projection, the causal short-key attention at
two 64-wide heads, the residual folds, both epilogue activations and the bias-free projection of the pooled row.

Bound: a floating-point network with no reference counterpart.  The oracle is the same network built from stock torch
modules (tests/text_ref.py) in FP32 on the CPU with the same weights upcast; the yardstick for "as good as FP16 can be"
is that stock network run in FP16 on the GPU.  Required, per output: max |ours - fp32| <= 1.5 x max |stock fp16 - fp32|
(the margin of tests/test_vae_gpu.py), with a floor of one FP16 ulp of the output range.
"""
import numpy as np
import pytest
import torch

from tests import text_ref
from tests.test_sampler_gpu import tiny  # noqa: F401  (the tiny W8A8 UNet of the sampler tests, as a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L_TINY = 32
OUTPUTS = ("last_hidden_state", "penultimate", "pooled")


def bits(t):
    return t.contiguous().view(torch.int16)


def small_cfg(act, proj):
    from mixdq_amd import text as T
    return dict(T.CLIP_L_CONFIG, hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512,
                vocab_size=1000, hidden_act=act, projection_dim=64 if proj else None)


def make_ids(B, T, vocab, seed):
    """Random ids below vocab - 1 with the maximum (the EOS token, vocab - 1) at a different position per row."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    ids = torch.randint(0, vocab - 1, (B, T), generator=g)
    for b in range(B):
        ids[b, (3 + 7 * b) % T] = vocab - 1
    return ids


@pytest.fixture(scope="module")
def small():
    """(activation, projection) -> encoder, and per T the ids with this path's outputs, computed once."""
    from mixdq_amd import text as T
    out = {}
    for act, proj in (("quick_gelu", False), ("gelu", True), ("quick_gelu", True), ("gelu", False)):
        cfg = small_cfg(act, proj)
        enc = T.build_text_encoder(cfg, seed=11, device=DEV)
        runs = {}
        for Tn in (77, 20):
            ids = make_ids(2, Tn, cfg["vocab_size"], 12 + Tn).to(DEV)
            runs[Tn] = (ids, enc(ids))
        out[(act, proj)] = dict(cfg=cfg, enc=enc, runs=runs)
    torch.cuda.synchronize()
    return out


def test_embed_tokens_equals_the_stock_sum_and_clamps(C):
    g = torch.Generator(device="cpu").manual_seed(3)
    V, Cw, Tmax = 300, 136, 77
    tok = torch.randn(V, Cw, generator=g).half().to(DEV)
    pos = torch.randn(Tmax, Cw, generator=g).half().to(DEV)
    for B, T in ((1, 1), (2, 77), (3, 20)):
        ids = torch.randint(0, V, (B, T), generator=g).to(torch.int32).to(DEV)
        want = (tok[ids.long()].float() + pos[:T].float()).half()
        assert torch.equal(bits(C.embed_tokens_f16(ids, tok, pos)), bits(want)), (B, T)
    ids = torch.tensor([[0, V - 1, V, V + 5000, -1, -2 ** 31, 2 ** 31 - 1, 5]], dtype=torch.int32, device=DEV)
    want = (tok[ids.long().clamp(0, V - 1)].float() + pos[:8].float()).half()
    assert torch.equal(bits(C.embed_tokens_f16(ids, tok, pos)), bits(want))
    with pytest.raises(RuntimeError):
        C.embed_tokens_f16(ids.long(), tok, pos)                      # int64 ids are the caller's to convert
    with pytest.raises(RuntimeError):
        C.embed_tokens_f16(torch.zeros(1, 78, dtype=torch.int32, device=DEV), tok, pos)     # T > Tmax


@pytest.mark.parametrize("act,proj", [("quick_gelu", False), ("gelu", True), ("quick_gelu", True), ("gelu", False)])
@pytest.mark.parametrize("Tn", (77, 20))
def test_text_encoder_vs_the_stock_network(small, act, proj, Tn):
    s = small[(act, proj)]
    cfg, enc = s["cfg"], s["enc"]
    ids, ours = s["runs"][Tn]
    C = cfg["hidden_size"]
    assert tuple(ours.last_hidden_state.shape) == (2, Tn, C) and tuple(ours.penultimate.shape) == (2, Tn, C)
    assert tuple(ours.pooled.shape) == (2, 64 if proj else C)
    sd = enc.state_dict()
    ref = text_ref.stock_encoder(cfg, sd, torch.float32, "cpu")(ids.cpu())
    stock16 = text_ref.stock_encoder(cfg, sd, torch.float16, DEV)(ids)
    for name, o, r, s16 in zip(OUTPUTS, ours, ref, stock16):
        assert o.dtype == torch.float16 and bool(torch.isfinite(o).all())
        err_ours = (o.float().cpu() - r).abs().max().item()
        err_stock = (s16.float().cpu() - r).abs().max().item()
        amax = r.abs().max().item()
        ulp = 2.0 ** (np.floor(np.log2(amax)) - 10)                   # one FP16 ulp at the top of the output range
        print(f"text small {act} proj={proj} T={Tn} {name}: max |ref| {amax:.4f}, max err ours {err_ours:.3e}, "
              f"stock fp16 {err_stock:.3e}, ulp floor {ulp:.3e}")
        assert amax > 1e-2
        assert err_ours <= max(1.5 * err_stock, ulp), name
    # int32 ids are taken as they are
    again = enc(ids.to(torch.int32))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, ours))


def test_text_graph_replay_equals_eager_bit_for_bit(small):
    from mixdq_amd import text as T
    from mixdq_amd.quantize_sdxl import hip_graph_opt
    s = small[("gelu", True)]
    ids, want = s["runs"][77]
    enc = hip_graph_opt(T.build_text_encoder(s["cfg"], seed=11, device=DEV))
    first = [o.clone() for o in enc(ids)]
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first, want))
    other = ids.flip(0).contiguous()                                   # the same graph on other ids: the EOS rows move
    eager = s["enc"](other)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(enc(other), eager))
    assert len(enc.forward._cached) == 1


def test_text_batch_row_equals_the_sequence_alone(small):
    for key in (("quick_gelu", False), ("gelu", True)):
        s = small[key]
        for Tn in (77, 20):
            ids, out = s["runs"][Tn]
            for b in range(2):
                alone = s["enc"](ids[b:b + 1])
                for name, a, o in zip(OUTPUTS, alone, out):
                    assert torch.equal(bits(a), bits(o[b:b + 1])), (key, Tn, b, name)


def test_text_forward_runs_this_librarys_launches_only(small):
    """Traced three ways.  `_C`'s launch recorder sees the INT8 GEMM / conv entry points and the attention launches
    only -- not linear_f16, layernorm_quantize or embed_tokens_f16, which are most of this forward -- so on its own it
    could not show that nothing else runs: it records one attention launch per layer here and nothing besides.  The
    check that covers every launch is the other two: the torch operators a forward dispatches are the id conversion,
    the argmax / gather of the pooled row, views and allocations -- nothing that computes on the hidden states; and
    the device kernels of a forward are this library's, apart from those few operators' own."""
    from torch.profiler import ProfilerActivity, profile
    from torch.utils._python_dispatch import TorchDispatchMode
    from mixdq_amd import _C
    s = small[("gelu", True)]
    enc, (ids, _) = s["enc"], s["runs"][77]
    assert _C.RECORD is None
    _C.RECORD = []
    try:
        enc(ids)
        recorded = [e[0] for e in _C.RECORD]
    finally:
        _C.RECORD = None
    assert recorded == ["attention"] * s["cfg"]["num_hidden_layers"], recorded
    seen = []

    class Rec(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(func.overloadpacket.__name__)
            return func(*args, **(kwargs or {}))
    with Rec():
        enc(ids)
    allowed = {"_to_copy", "clone", "contiguous", "argmax", "gather", "empty", "empty_like", "empty_strided",
               "view", "_unsafe_view", "reshape", "expand", "slice", "select", "detach", "alias", "as_strided", "squeeze",
               "unsqueeze"}
    assert set(seen) <= allowed, sorted(set(seen) - allowed)
    assert seen.count("argmax") == 1 and seen.count("gather") == 1 and seen.count("_to_copy") == 1
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        enc(ids)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
             and "Memcpy" not in e.name and "Memset" not in e.name]
    ours = [n for n in names if "mixdq" in n]
    other = [n for n in names if "mixdq" not in n]
    layers = s["cfg"]["num_hidden_layers"]
    assert len(ours) == 1 + 7 * layers + 1 + 1, ours                  # embed, 7 per layer, final norm, projection
    assert len(other) <= 3, other                                    # the id conversion, argmax, gather
    assert sum("attn_short_kernel" in n for n in ours) == layers
    assert sum("embed_tokens_kernel" in n for n in ours) == 1


def test_text_encoder_refusals(small):
    from mixdq_amd import text as T
    s = small[("gelu", True)]
    enc = s["enc"]
    with pytest.raises(RuntimeError, match="1 <= T <= 77"):
        enc(torch.zeros(1, 78, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        enc(torch.zeros(1, 77, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        enc(torch.zeros(1, 77, dtype=torch.float16, device=DEV))
    fp32 = T.build_text_encoder(s["cfg"], seed=11, device=DEV, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="TextEncoder.forward: the encoder runs in FP16"):
        fp32(torch.zeros(1, 77, dtype=torch.int64, device=DEV))
    mixed = T.build_text_encoder(s["cfg"], seed=11, device=DEV)          # one FP32 layer in an FP16 encoder
    mixed.text_model.encoder.layers[1].mlp.fc2.float()
    with pytest.raises(RuntimeError, match="TextEncoder.forward: the encoder runs in FP16"):
        mixed(torch.zeros(1, 77, dtype=torch.int64, device=DEV))


def test_text_graph_replay_sees_a_later_load_state_dict(small):
    """A captured forward holds the addresses of the parameters AND of the cached q|k|v tensors derived from them;
    load_state_dict rewrites both in place, so a replay computes with the new weights."""
    from mixdq_amd import text as T
    from mixdq_amd.quantize_sdxl import hip_graph_opt
    s = small[("quick_gelu", True)]
    ids, _ = s["runs"][20]
    enc = T.build_text_encoder(s["cfg"], seed=11, device=DEV)
    donor = T.build_text_encoder(s["cfg"], seed=12, device=DEV)
    want = donor(ids)
    g = hip_graph_opt(enc)
    before = [o.clone() for o in g(ids)]
    ptrs = [w.data_ptr() for w, _ in enc._derived().values()]
    enc.load_state_dict(donor.state_dict())
    assert [w.data_ptr() for w, _ in enc._derived().values()] == ptrs
    after = g(ids)
    assert len(g.forward._cached) == 1                                 # a replay, not a new capture
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(after, want))
    assert not torch.equal(bits(after[0]), bits(before[0]))


def test_encode_sdxl_feeds_the_sampler(tiny):  # noqa: F811
    from mixdq_amd import Sampler
    from mixdq_amd import text as T
    from mixdq_amd.quantize_sdxl import example_inputs
    base = dict(T.CLIP_L_CONFIG, num_hidden_layers=1, intermediate_size=256, vocab_size=1000)
    enc_l = T.build_text_encoder(dict(base, hidden_size=768, num_attention_heads=12), seed=5, device=DEV)
    enc_g = T.build_text_encoder(dict(base, hidden_size=1280, num_attention_heads=20, hidden_act="gelu",
                                      projection_dim=1280), seed=6, device=DEV)
    ids_l, ids_g = make_ids(1, 77, 1000, 31).to(DEV), make_ids(1, 77, 1000, 32).to(DEV)
    ehs, emb = T.encode_sdxl(enc_l, enc_g, ids_l, ids_g)
    out_l, out_g = enc_l(ids_l), enc_g(ids_g)
    assert tuple(ehs.shape) == (1, 77, 2048) and tuple(emb.shape) == (1, 1280) and ehs.dtype == emb.dtype == torch.float16
    assert torch.equal(bits(ehs[..., :768]), bits(out_l.penultimate))
    assert torch.equal(bits(ehs[..., 768:]), bits(out_g.penultimate))
    assert torch.equal(bits(emb), bits(out_g.pooled))
    eos = int(ids_g[0].argmax())
    want = C_linear(out_g.last_hidden_state[:, eos], enc_g.text_projection.weight)
    assert torch.equal(bits(emb), bits(want))
    assert torch.equal(bits(T.encode_sd15(enc_l, ids_l)), bits(out_l.last_hidden_state))
    sm = Sampler(tiny, "euler", 2)
    inp = example_inputs(1, L_TINY, DEV, seed=21)
    noise = torch.randn(1, 4, L_TINY, L_TINY, generator=torch.Generator(device="cpu").manual_seed(22)).to(DEV)
    added = dict(inp["added_cond_kwargs"], text_embeds=emb)
    latents = sm.sample(noise, ehs, added)
    assert tuple(latents.shape) == (1, 4, L_TINY, L_TINY) and bool(torch.isfinite(latents).all())
    other = sm.sample(noise, inp["encoder_hidden_states"], inp["added_cond_kwargs"])
    assert not torch.equal(latents, other)                             # (the conditioning reaches the UNet)


def C_linear(x, w):
    from mixdq_amd import _C
    return _C.linear_f16(x.contiguous(), w, None)
