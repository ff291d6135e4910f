"""Host tests of mixdq_amd.text (no GPU): the encoders' parameter inventory against transformers' CLIPTextModel names,
the state-dict round trip, the derived-weight cache, the quick-GELU specification and the binding's documented
clamp."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from mixdq_amd import text as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(T.CLIP_L_CONFIG, hidden_size=128, num_attention_heads=2, num_hidden_layers=3, intermediate_size=512,
             vocab_size=1000)
SMALL_PROJ = dict(SMALL, hidden_act="gelu", projection_dim=64)


def _meta(cfg):
    with torch.device("meta"):
        return T.TextEncoder(cfg)


@pytest.mark.parametrize("cfg,total", [(T.CLIP_L_CONFIG, 123_060_480), (T.OPENCLIP_BIGG_CONFIG, 694_659_840)])
def test_parameter_names_and_counts_of_the_full_configs(cfg, total):
    listed = T.state_dict_names(cfg)
    assert T.parameter_count(cfg) == total
    enc = _meta(cfg)                                                  # shapes only: nothing is allocated
    assert {n: tuple(p.shape) for n, p in enc.named_parameters()} == dict(listed)
    assert len(listed) == len(dict(listed))
    assert sum(p.numel() for p in enc.parameters()) == total
    counts = T.parameter_counts(enc)
    proj = cfg["projection_dim"] * cfg["hidden_size"] if cfg.get("projection_dim") else 0
    assert counts["text_projection"] == proj and counts["text_model"] == total - proj
    L = cfg["num_hidden_layers"] - 1
    for s in ("layer_norm1", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj",
              "layer_norm2", "mlp.fc1", "mlp.fc2"):
        assert f"text_model.encoder.layers.{L}.{s}.weight" in dict(listed)
        assert f"text_model.encoder.layers.{L}.{s}.bias" in dict(listed)
    assert ("text_projection.weight" in dict(listed)) == bool(cfg.get("projection_dim"))
    assert "text_projection.bias" not in dict(listed)


def test_configs_are_the_published_ones():
    l, g = T.CLIP_L_CONFIG, T.OPENCLIP_BIGG_CONFIG
    assert (l["hidden_size"], l["num_hidden_layers"], l["num_attention_heads"], l["intermediate_size"],
            l["hidden_act"], l["projection_dim"]) == (768, 12, 12, 3072, "quick_gelu", None)
    assert (g["hidden_size"], g["num_hidden_layers"], g["num_attention_heads"], g["intermediate_size"],
            g["hidden_act"], g["projection_dim"]) == (1280, 32, 20, 5120, "gelu", 1280)
    for c in (l, g):
        assert (c["vocab_size"], c["max_position_embeddings"], c["layer_norm_eps"]) == (49408, 77, 1e-5)


@pytest.mark.parametrize("cfg", (SMALL, SMALL_PROJ))
def test_keys_equal_transformers_clip_text_model(cfg, tmp_path):
    tr = pytest.importorskip("transformers")
    tc = tr.CLIPTextConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"],
                           intermediate_size=cfg["intermediate_size"], num_hidden_layers=cfg["num_hidden_layers"],
                           num_attention_heads=cfg["num_attention_heads"], hidden_act=cfg["hidden_act"],
                           max_position_embeddings=cfg["max_position_embeddings"],
                           projection_dim=cfg.get("projection_dim") or 512, layer_norm_eps=cfg["layer_norm_eps"])
    cls = tr.CLIPTextModelWithProjection if cfg.get("projection_dim") else tr.CLIPTextModel
    # The names under test are those of the published checkpoint FILES (`text_model.*`, `text_projection.weight`), and
    # the judge of them is transformers' own loader: this encoder's state dict is written out as a checkpoint in a
    # local directory and loaded with from_pretrained, which must find every tensor it wants and none it does not.
    # Nothing is prefixed or mapped here -- the module tree of a transformers version need not carry the
    # `text_model.` level itself (5.x maps the file's names onto its modules when it loads).
    safetensors = pytest.importorskip("safetensors.torch")
    ours = T.build_text_encoder(cfg)
    sd = ours.state_dict()
    assert {n: tuple(v.shape) for n, v in sd.items()} == dict(T.state_dict_names(cfg))
    tc.save_pretrained(str(tmp_path))
    safetensors.save_file({n: v.contiguous() for n, v in sd.items()}, os.path.join(str(tmp_path), "model.safetensors"))
    model, info = cls.from_pretrained(str(tmp_path), local_files_only=True, output_loading_info=True)
    assert not info["missing_keys"] and not info["unexpected_keys"], info
    assert not info.get("mismatched_keys") and not info.get("error_msgs"), info
    theirs = model.state_dict()
    assert sum(v.numel() for v in theirs.values() if v.is_floating_point()) >= T.parameter_count(cfg)
    for n, v in sd.items():                                           # (values arrive where the name says)
        t = theirs[n] if n in theirs else theirs[n[len("text_model."):]]
        assert tuple(t.shape) == tuple(v.shape) and torch.equal(t.to(v.dtype), v), n
    # and the other way: what transformers holds loads into this encoder under its checkpoint names
    back = T.build_text_encoder(cfg, seed=7)
    back.load_state_dict({n: (theirs[n] if n in theirs else theirs[n[len("text_model."):]]).half() for n in sd},
                         strict=True)


def test_state_dict_round_trip_and_synthetic_weights():
    a, b = T.build_text_encoder(SMALL_PROJ, seed=1), T.build_text_encoder(SMALL_PROJ, seed=2)
    assert all(p.dtype == torch.float16 for p in a.parameters()) and not a.training
    sa = a.state_dict()
    assert set(sa) == {n for n, _ in T.state_dict_names(SMALL_PROJ)}
    assert not torch.equal(sa["text_model.encoder.layers.0.mlp.fc1.weight"],
                           b.state_dict()["text_model.encoder.layers.0.mlp.fc1.weight"])
    b.load_state_dict(sa, strict=True)
    for k, v in b.state_dict().items():
        assert torch.equal(v, sa[k]), k
    again = T.build_text_encoder(SMALL_PROJ, seed=1).state_dict()
    assert all(torch.equal(again[k], sa[k]) for k in sa)


def test_derived_qkv_cache_is_rebuilt_after_a_load_and_a_move():
    a, b = T.build_text_encoder(SMALL, seed=1), T.build_text_encoder(SMALL, seed=2)
    d0 = a._derived()
    assert all(a._derived()[i] is d0[i] for i in d0) and len(d0) == len(a.text_model.encoder.layers)   # cached
    w, bias = d0[1]
    att = a.text_model.encoder.layers[1].self_attn
    assert tuple(w.shape) == (384, 128) and tuple(bias.shape) == (384,)
    assert torch.equal(w[:128], att.q_proj.weight) and torch.equal(w[128:256], att.k_proj.weight)
    assert torch.equal(w[256:], att.v_proj.weight) and torch.equal(bias[128:256], att.k_proj.bias)
    # a load rewrites the derived tensors where they are (a captured graph holds their addresses) ...
    ptrs = [(w.data_ptr(), bias.data_ptr()) for w, bias in d0.values()]
    a.load_state_dict(b.state_dict())
    d1 = a._derived()
    assert [(w.data_ptr(), bias.data_ptr()) for w, bias in d1.values()] == ptrs
    for layer, (w, bias) in zip(b.text_model.encoder.layers, d1.values()):
        bw, bb = layer.self_attn.qkv()
        assert torch.equal(w, bw) and torch.equal(bias, bb)
    assert not torch.equal(d1[1][0][:128], T.build_text_encoder(SMALL, seed=1).text_model.encoder.layers[1]
                           .self_attn.q_proj.weight)
    # ... also before the cache exists, and through assign=True, which swaps the parameters themselves
    c = T.build_text_encoder(SMALL, seed=3)
    c.load_state_dict(b.state_dict())
    assert torch.equal(c._derived()[2][0], d1[2][0])
    c.load_state_dict(T.build_text_encoder(SMALL, seed=1).state_dict(), assign=True)
    assert torch.equal(c._derived()[1][0][:128], T.build_text_encoder(SMALL, seed=1).text_model.encoder
                       .layers[1].self_attn.q_proj.weight)
    # a move or a dtype change drops them: every tensor has a new address anyway
    a.to(torch.float32)
    d2 = a._derived()
    assert d2[0] is not d1[0] and d2[0][0].dtype == torch.float32
    assert torch.equal(d2[1][0][:128], a.text_model.encoder.layers[1].self_attn.q_proj.weight)


def test_forward_refusals_without_a_gpu():
    enc = T.build_text_encoder(SMALL)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        enc(torch.zeros(1, 77, dtype=torch.int64))                    # CPU ids
    with pytest.raises(ValueError):
        T.TextEncoder(dict(SMALL, num_attention_heads=4))             # heads not 64 wide
    with pytest.raises(ValueError):
        T.TextEncoder(dict(SMALL, hidden_act="relu"))


def test_quick_gelu_specification_vs_float64(tmp_path):
    """mixdq_quick_geluf, compiled from include/mixdq_math.h by the host compiler without contraction, against
    x / (1 + exp(-1.702 x)) in float64, within 2 FP32 ulps.

    The grid: the specification rounds the product t = 1.702 x to FP32 before the exp, which perturbs e = exp(-t) by
    a relative |t| 2^-24 -- |t| / 2 ulps of e -- and that reaches the result scaled by s = e / (1 + e).  The float64
    formula is a 2-ulp yardstick only where s |t| stays below one (half an ulp from this term): for x >= 0,
    s |t| = t / (1 + e^t) <= 0.28 everywhere; for x < 0, |t| sigmoid(|t|) <= 1 up to |t| = 1.27, x >= -0.75.  So the
    grid is [-0.75, 12] and the positive FP16 range.  On the negative tail [-12, -0.75) the product's rounding
    dominates (4 ulps at x = -12) and says nothing about the code: there the yardstick is the same formula on the
    FP32-rounded product, with 3 ulps (mixdq_expf's 2, at s ~ 1, plus half an ulp each for the sum and the division)."""
    src = tmp_path / "qg.c"
    src.write_text('#include "mixdq_math.h"\nfloat quick_geluf(float x) { return mixdq_quick_geluf(x); }\n')
    lib = tmp_path / "libqg.so"
    subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                           "-I", os.path.join(ROOT, "include"), "-o", str(lib), str(src), "-lm"])
    L = ctypes.CDLL(str(lib))
    L.quick_geluf.argtypes, L.quick_geluf.restype = [ctypes.c_float], ctypes.c_float

    def ulps(grid, rounded_product):
        got = np.array([L.quick_geluf(float(x)) for x in grid], np.float32).astype(np.float64)
        x64 = grid.astype(np.float64)
        t = (np.float32(1.702) * grid).astype(np.float64) if rounded_product else np.float32(1.702).astype(np.float64) * x64
        want = x64 / (1.0 + np.exp(-t))
        assert (np.abs(want[grid != 0]) >= 2.0 ** -126).all()          # (the grid stays in the normal range)
        return np.abs(got - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)

    main = np.concatenate([np.linspace(-0.75, 12, 5101), [30.0, 60.0, 1e-3, -1e-3, 1e-6, -1e-6],
                           np.arange(100.0, 65504.0, 4093.5), [65504.0]]).astype(np.float32)
    tail = np.linspace(-12, -0.75, 2251).astype(np.float32)
    e_main, e_tail = ulps(main, False).max(), ulps(tail, True).max()
    print(f"quick-GELU vs float64: {e_main:.2f} ulp on the main grid, {e_tail:.2f} ulp on the negative tail")
    assert e_main <= 2.0
    assert e_tail <= 3.0
    assert L.quick_geluf(0.0) == 0.0 and np.isnan(L.quick_geluf(float("nan")))


def test_embedding_clamp_is_documented():
    from mixdq_amd import _C
    doc = _C.embed_tokens_f16.__doc__
    assert "clamped" in doc and "[0, V)" in doc
    header = open(os.path.join(ROOT, "include", "mixdq_hip.h")).read()
    i = header.index("Token + position embedding of a text encoder")
    assert "CLAMPED" in header[i:header.index("int mixdq_embed_tokens_f16", i)]
    for name in ("MIXDQ_FLAG_CAUSAL = 32", "MIXDQ_FLAG_ACT_GELU = 64", "MIXDQ_FLAG_ACT_QUICK_GELU = 128",
                 "#define MIXDQ_ABI_VERSION 3"):
        assert name in header
    assert (_C.FLAG_CAUSAL, _C.FLAG_ACT["gelu"], _C.FLAG_ACT["quick_gelu"]) == (32, 64, 128)
