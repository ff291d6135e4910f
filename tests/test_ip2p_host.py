"""InstructPix2Pix on the host: the three-row guidance's restatement (tests/ip2p_ref.py) against a float64 formula and
against the compiled specification (include/mixdq_math.h under a host compiler), the argument checks of the two new
entry points on a CPU-only load, the 8-channel configs and the Sampler's constructor, and the split conv_in of an
8-channel UNet in float64."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import ip2p_ref as P
from tests import multistep_ref as M
from tests import sampler_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _triples(seed, n=4099):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(n).astype(np.float16) for _ in range(3))


# ---- 1. the restatement against float64, and against the two-row guidance ----------------------------------------
@pytest.mark.parametrize("g,gi", [(7.5, 1.5), (1.0, 1.0), (12.0, 0.25), (0.0, 3.0)])
def test_guided_eps3_against_the_float64_formula(g, gi):
    """Six roundings, each at most u = 2^-24 relative to its result; every intermediate result is bounded by
    |e_u| + |g| |e_t - e_i| + |gi| |e_i - e_u| (the two differences of FP16 values are exact in FP32)."""
    e_t, e_i, e_u = _triples(11)
    got = P.guided_eps3(e_t, e_i, e_u, g, gi)
    assert got.dtype == np.float32 and got.shape == (4099,)
    t, i, u_ = (v.astype(np.float64) for v in (e_t, e_i, e_u))
    g64, gi64 = float(f32(g)), float(f32(gi))
    want = u_ + g64 * (t - i) + gi64 * (i - u_)
    u = 2.0 ** -24
    bound = 6 * u * (np.abs(u_) + abs(g64) * np.abs(t - i) + abs(gi64) * np.abs(i - u_))
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    if g == 7.5:
        assert np.abs(want).max() > 10.0 and (err > 0).any()          # the check sees real roundings


@pytest.mark.parametrize("gi", [0.0, 1.5, -3.25, 1e30])
def test_guided_eps3_with_equal_image_and_unconditional_rows_is_the_two_row_guidance(gi):
    e_t, _, e_u = _triples(12)
    e_u[:4] = np.array([0.0, -0.0, 65504.0, -65504.0], dtype=np.float16)
    g = 7.5
    got = P.guided_eps3(e_t, e_u.copy(), e_u, g, gi)
    want_m = M.guided(e_u, e_t, g)
    zeros = np.zeros(e_u.shape, dtype=f32)
    want_r, _ = R.step(zeros, e_u, e_t, (0.0, 1.0, 0.0, 1.0), g)       # 0 * x + 1 * e: sampler_ref's own guidance
    assert np.array_equal(got, want_m) and np.array_equal(got, want_r)
    assert np.isfinite(got).all()


# ---- 2. the compiled specification ---------------------------------------------------------------------------------
_MAIN = r"""
#include <stdio.h>
#include "mixdq_math.h"

/* spec IN OUT: IN holds FP32 tuples (e_t, e_i, e_u, g, gi), OUT one FP32 per tuple */
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 3;
  float t[5];
  while (fread(t, 4, 5, in) == 5) {
    const float r = mixdq_sampler_guided_eps3(t[0], t[1], t[2], t[3], t[4]);
    fwrite(&r, 4, 1, out);
  }
  fclose(in);
  return fclose(out) ? 4 : 0;
}
"""


def test_compiled_guided_eps3_equals_the_restatement(tmp_path):
    src, exe = tmp_path / "spec.c", tmp_path / "spec"
    src.write_text(_MAIN)
    subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src), "-lm"])
    rng = np.random.default_rng(13)
    n = 4099
    t = np.empty((n, 5), dtype=f32)
    t[:, :3] = rng.standard_normal((n, 3)).astype(np.float16)
    t[:, 3] = rng.choice(np.array([7.5, 1.0, 5.0, 12.0, 0.0], dtype=f32), n)
    t[:, 4] = rng.choice(np.array([1.5, 1.0, 0.0, 2.25, 1.2], dtype=f32), n)
    inf = f32(np.inf)
    edge = np.array([[0.0, -0.0, -0.0, 7.5, 1.5], [-0.0, -0.0, 0.0, 7.5, 1.5], [65504.0, -65504.0, 65504.0, 7.5, 1.5],
                     [inf, 1.0, 1.0, 7.5, 1.5], [1.0, inf, 1.0, 7.5, 1.5], [1.0, 1.0, np.nan, 7.5, 1.5],
                     [3e38, -3e38, 1.0, 7.5, 1.5], [6e-8, -6e-8, 6e-8, 7.5, 1.5],
                     [1.0, 1.0 - 2.0 ** -11, 2.0 ** -24, 1.0, 1.0]], dtype=f32)
    t = np.concatenate([t, edge])
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.ascontiguousarray(t).tofile(fin)
    subprocess.check_call([str(exe), str(fin), str(fout)])
    got = np.fromfile(fout, dtype=f32)
    want = np.concatenate([P.guided_eps3(r[0:1], r[1:2], r[2:3], r[3], r[4]) for r in t])
    assert got.shape == want.shape == (len(t),)
    both_nan = np.isnan(got) & np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[~both_nan], want.view(np.uint32)[~both_nan])
    assert both_nan.sum() >= 3


# ---- 3. the C ABI -----------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points_and_rejects_bad_arguments():
    """CPU-only load: the argument checks run on the host before any launch (no pointer below is dereferenced)."""
    from mixdq_amd.build import build
    lib = ctypes.CDLL(build())
    assert hasattr(lib, "mixdq_sampler_step3") and hasattr(lib, "mixdq_ip2p_cond_f16")
    vp, i64, i32, fl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    fn = lib.mixdq_sampler_step3
    fn.argtypes = [vp, vp, vp, vp, i32, vp, i32, vp, vp, fl, fl, i64, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp, i32, vp,
                   vp]
    fn.restype = i32
    p = 0x1000
    ok = dict(x=p, eps=p, inp=p, table=p, width=4, t_table=p, n_steps=4, step=p, timestep=p, g=7.5, gi=1.5, n=64,
              row_stride=64, noise=None, noise_stride=0, seeds=None, n_image=0, hist=None, first=None, z=None,
              noise0=None, mask=None, channels=4, blend=None)

    def call(**kw):
        a = dict(ok, **kw)
        assert set(a) == set(ok)
        return fn(*[a[k] for k in ok], None)
    for bad in (dict(x=None), dict(eps=None), dict(inp=None), dict(table=None), dict(t_table=None), dict(step=None),
                dict(timestep=None),                                        # a null base pointer
                dict(row_stride=56),                                        # row_stride < n
                dict(n=-1), dict(n_steps=0),
                dict(width=5), dict(width=0),                               # the table is coef or coef8
                dict(width=8, hist=0x2000, first=p, noise=p, noise_stride=64),      # width 8 with noise
                dict(width=8, hist=0x2000, first=p, seeds=p, n_image=64),           # ... or seeds
                dict(noise=p, noise_stride=64, seeds=p, n_image=64),        # noise and seeds together
                dict(width=8), dict(width=8, first=p), dict(width=8, hist=0x2000),  # width 8 without hist / first
                dict(hist=0x2000, first=p),                                 # ... and hist without width 8
                dict(width=8, hist=p, first=p),                             # the history overlaps the state
                dict(seeds=p, n_image=48),                                  # n % n_image
                dict(z=p, noise0=p, mask=p),                                # a masked step without its table
                dict(z=p, noise0=p, mask=p, blend=p, channels=5)):          # n % channels
        assert call(**bad) == 1, bad
    for bad in (dict(x=p + 4), dict(eps=p + 2), dict(inp=p + 8), dict(table=p + 4),     # a misaligned state, ...
                dict(n=67, row_stride=68),                                  # row_stride % 8 != 0
                dict(noise=p, noise_stride=66),
                dict(seeds=p + 4, n_image=64),
                dict(width=8, hist=0x2008, first=p),
                dict(z=p + 4, noise0=p, mask=p, blend=p)):
        assert call(**bad) == 2, bad

    cond = lib.mixdq_ip2p_cond_f16
    cond.argtypes = [vp, vp, i32, i64, i32, i32, fl, vp]
    cond.restype = i32
    for args in ((0x1000, 0x3000, 2, 4, 4, 2), (0x1000, 0x3000, 2, 4, 4, 0), (0x1000, 0x3000, 2, 4, 4, 4),     # rows
                 (0x1000, 0x3000, 2, 4, 9, 3), (0x1000, 0x3000, 2, 4, 0, 3),                                    # L
                 (None, 0x3000, 2, 4, 4, 3), (0x1000, None, 2, 4, 4, 3), (0x1000, 0x3000, -1, 4, 4, 3),
                 (0x1000, 0x3000, 2, -4, 4, 3)):
        assert cond(*args, 1.0, None) == 1, args
    for args in ((0x1000, 0x3008, 2, 4, 4, 3), (0x1001, 0x3000, 2, 4, 4, 3)):
        assert cond(*args, 1.0, None) == 2, args
    assert cond(None, None, 0, 16, 4, 3, 1.0, None) == 0 and cond(None, None, 2, 0, 4, 1, 1.0, None) == 0
    lib.mixdq_abi_version.restype = i32
    assert lib.mixdq_abi_version() == 3


def test_bindings_exist_and_refuse_before_any_device_work():
    from mixdq_amd import _C
    assert callable(_C.sampler_step3) and callable(_C.ip2p_cond)
    with pytest.raises(RuntimeError, match="moments should be"):
        _C.ip2p_cond(torch.zeros(1, 8, 4, 4, dtype=torch.float16))           # not on a GPU
    x = torch.zeros(64)
    with pytest.raises(RuntimeError, match="coef8 comes with hist and first"):
        _C.sampler_step3(x, x, x, torch.zeros(3, 8), x, x, x, 7.5, 1.5)
    with pytest.raises(RuntimeError, match="go together"):
        _C.sampler_step3(x, x, x, torch.zeros(3, 4), x, x, x, 7.5, 1.5, z=x)


# ---- 4. configs and constructor -------------------------------------------------------------------------------------
def _meta(cfg):
    from mixdq_amd.unet import SDXLUNet
    with torch.device("meta"):
        return SDXLUNet(cfg)


def test_ip2p_configs():
    from mixdq_amd.unet import SD15_CONFIG, SD15_IP2P_CONFIG, SDXL_CONFIG, SDXL_IP2P_CONFIG
    for cfg, base, total in ((SD15_IP2P_CONFIG, SD15_CONFIG, 859_532_484), (SDXL_IP2P_CONFIG, SDXL_CONFIG, 2_567_475_204)):
        assert cfg == dict(base, in_channels=8)
        u = _meta(cfg)
        c0 = cfg["block_out_channels"][0]
        assert u.cond_channels == 4 and tuple(u.conv_in.weight.shape) == (c0, 8, 3, 3)
        assert sum(p.numel() for p in u.parameters()) == total
        assert sum(p.numel() for p in _meta(base).parameters()) == total - c0 * 4 * 9


def test_sampler_constructor_and_instruct_signature():
    import inspect
    from mixdq_amd.sampler import Sampler
    sm = Sampler(None, "euler", 3, 7.5, image_guidance_scale=1.5)
    assert sm.rows_per_image == 3 and sm.guidance_scale == 7.5 and sm.image_guidance_scale == 1.5
    assert Sampler(None, "euler", 3, 7.5).rows_per_image == 2 and Sampler(None, "euler", 3, 7.5).image_guidance_scale is None
    assert Sampler(None, "euler", 3, 1.0, image_guidance_scale=1.0).rows_per_image == 3      # three rows whatever the scales
    assert Sampler(None, "lcm", 4).rows_per_image == 1
    par = inspect.signature(Sampler.__init__).parameters
    assert list(par)[:7] == ["self", "unet", "kind", "n_steps", "guidance_scale", "spacing", "karras"]
    assert par["image_guidance_scale"].kind is inspect.Parameter.KEYWORD_ONLY and par["image_guidance_scale"].default is None
    ins = inspect.signature(Sampler.instruct).parameters
    assert list(ins) == ["self", "enc", "dec", "image", "noise", "encoder_hidden_states", "added_cond_kwargs",
                         "step_noise", "seed", "cond_scale"]
    assert all(ins[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("step_noise", "seed", "cond_scale"))
    assert ins["cond_scale"].default == 1.0 and ins["added_cond_kwargs"].default is None


# ---- 5. the split conv_in of an 8-channel UNet in float64 ----------------------------------------------------------
def test_split_forward_equals_the_concatenated_one_in_float64():
    import bench
    from mixdq_amd.quantize_sdxl import example_inputs
    from mixdq_amd.unet import SDXLUNet, init_synthetic_weights
    unet = init_synthetic_weights(SDXLUNet(dict(bench.TINY_CFG, in_channels=8)), seed=3).double().eval()
    assert unet.cond_channels == 4
    inp = example_inputs(2, 8, "cpu", in_channels=8, seed=4)
    to64 = lambda v: v.double() if torch.is_tensor(v) else {k: t.double() for k, t in v.items()}   # noqa: E731
    inp = {k: to64(v) for k, v in inp.items()}
    rest = (inp["timestep"], inp["encoder_hidden_states"], inp["added_cond_kwargs"])
    g = torch.Generator().manual_seed(9)
    cat8 = torch.randn(2, 8, 8, 8, generator=g, dtype=torch.float64)
    x4, c = cat8[:, :4].contiguous(), cat8[:, 4:].contiguous()
    with torch.no_grad():
        out_cat = unet(cat8, *rest)[0]
        term = unet.cond_term(c)
        out_split = unet(x4, *rest, cond_term=term)[0]
        # the unconditional block of a three-row run: a zero conditioning leaves conv_in's bias alone
        out_zero = unet(x4, *rest, cond_term=unet.cond_term(torch.zeros_like(c)))[0]
        out_zero_cat = unet(torch.cat([x4, torch.zeros_like(c)], dim=1), *rest)[0]
    assert tuple(term.shape) == (2, unet.conv_in.out_channels, 8, 8) and term.dtype == torch.float64
    d = (out_cat - out_split).abs().max().item()
    print(f"split vs concatenated, float64: max |d| {d:.3e}, output max {out_cat.abs().max().item():.3e}")
    assert float(out_cat.abs().max()) > 1e-3 and not torch.equal(out_cat, out_zero_cat)
    assert d <= 1e-12
    assert (out_zero - out_zero_cat).abs().max().item() <= 1e-12
    with pytest.raises(RuntimeError, match="needs cond_term"):
        unet(x4, *rest)
