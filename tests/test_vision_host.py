"""The vision encoder without a GPU: parameter names and count on the meta device, the head-width refusal, the entry
point's host-side refusals through ctypes, and the numpy restatement against a float64 convolution."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vision_ref


def test_vit_h_names_and_parameter_count_on_the_meta_device():
    from mixdq_amd import vision as V
    with torch.device("meta"):
        enc = V.VisionEncoder(V.CLIP_VIT_H_CONFIG)
    got = [(n, tuple(p.shape)) for n, p in enc.state_dict().items()]
    assert sorted(got) == sorted(V.state_dict_names(V.CLIP_VIT_H_CONFIG))
    n = V.parameter_count(V.CLIP_VIT_H_CONFIG)
    print(f"CLIP ViT-H/14 vision tower with projection: {n:,} parameters")
    assert n == sum(p.numel() for p in enc.parameters()) == 632_076_800          # the published 632 M
    assert V.parameter_count(V.CLIP_VIT_L_CONFIG) == 303_966_208                 # ViT-L/14: the published 304 M


def test_bigg_head_width_is_refused():
    from mixdq_amd import vision as V
    with torch.device("meta"), pytest.raises(ValueError, match="104"):
        V.VisionEncoder(dict(V.CLIP_VIT_H_CONFIG, hidden_size=1664, num_attention_heads=16))


@pytest.mark.parametrize("change,status", [
    (dict(image=None), 1), (dict(norm=None), 1), (dict(out=None), 1), (dict(ln_b=None), 1), (dict(dtype=3), 1),
    (dict(S=57), 9), (dict(S=14 * 33, rows=33 * 33 + 1), 9), (dict(N=96), 9), (dict(N=2112), 9), (dict(rows=16), 9),
    (dict(ldo=126), 9), (dict(weight=(1 << 20) + 8), 2), (dict(pos=(2 << 20) + 4), 2), (dict(), 0)])
def test_entry_point_refuses_on_the_host(change, status):
    """Dummy pointers: every refusal comes before the first HIP call (B = 0 for the accepted call: nothing to launch)."""
    from mixdq_amd.build import build
    lib = ctypes.CDLL(build())
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    fn = lib.mixdq_clip_patch_embed_f16
    fn.argtypes = [vp, i32] + [i64] * 4 + [vp] * 4 + [i32, vp, vp, ctypes.c_float, vp, i64] + [i32] * 3 + [vp]
    a = dict(image=1 << 24, dtype=0, norm=2 << 24, weight=3 << 24, cls=4 << 24, pos=5 << 24, rows=17, ln_w=6 << 24,
             ln_b=7 << 24, out=8 << 24, ldo=128, B=0, S=56, N=128)
    a.update(change)
    assert fn(a["image"], a["dtype"], 3 * a["S"] ** 2, a["S"] ** 2, a["S"], 1, a["norm"], a["weight"], a["cls"], a["pos"],
              a["rows"], a["ln_w"], a["ln_b"], 1e-5, a["out"], a["ldo"], a["B"], a["S"], a["N"], None) == status


def test_restatement_equals_a_float64_convolution():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 4, (2, 3, 28, 28)).astype(np.uint8)
    w = rng.integers(-1, 2, (64, 3, 14, 14)).astype(np.float16)
    cls, pos = (rng.integers(-8, 9, s).astype(np.float16) for s in ((64,), (5, 64)))
    e, acc, _ = vision_ref.embed(img, [(1, 0)] * 3, w, cls, pos)
    conv = F.conv2d(torch.from_numpy(img).double(), torch.from_numpy(w).double(), stride=14).flatten(2).transpose(1, 2)
    assert np.array_equal(acc, conv.numpy())
    assert np.array_equal(e[:, 1:].astype(np.float64), conv.numpy() + pos[1:]) and np.array_equal(e[0, 0], cls + pos[0])
