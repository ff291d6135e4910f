"""GPU tests of the patch-embed launch (csrc/clip_vision.hip) at every clip_patch_embed_kernel<MAXT>, each with spare
tiles (nt < MAXT) and without (nt == MAXT): exact inputs bit for bit, the LayerNorm epilogue on inputs that
tests/test_vision_widths_host.py shows to expose a wrong row sum, an output pitch above N, the largest grid, and float
pixels through the normalisation fma.

    MAXT   N run here (nt = N / 64)
       4   192 (3), 256 (4)
      12   320 (5), 576 (9), 768 (12)
      16   832 (13), 1024 (16)
      20   1088 (17), 1280 (20)
      32   1344 (21), 1728 (27), 2048 (32)
"""
import numpy as np
import pytest
import torch

from tests import vision_ref
from tests.test_vision_gpu import DEV, ONE, laid_out, launch, same, t
from tests.test_vision_widths_host import (ALL_N, EPS, LN_CASES, exact_inputs, fma_norms, fma_pixels, ln_inputs,
                                           ln_tolerance, maxt_of, one_tap_filter)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", ALL_N)
def test_exact_inputs_bit_for_bit_at_every_instantiation(C, N):
    """g = 5: one full block, a ragged block that spans patch rows, the class block; two images.  The ternary weights
    differ per column, so a permuted column or a spare tile's result in a real one changes bits."""
    g, B = 5, 2
    img, w, cls, pos = exact_inputs(g, N, B)
    want = vision_ref.embed(img, ONE, w, cls, pos)[0]
    assert np.abs(want.astype(np.float32)).max() < 2048
    for dtype, layout in ((torch.uint8, "contiguous"), (torch.float16, "sliced")):
        got = launch(C, laid_out(t(img).to(dtype), layout), ONE, w, cls, pos)
        assert got.shape == want.shape and same(got, want), (N, maxt_of(N), dtype, layout)


@pytest.mark.parametrize("g,N", LN_CASES)
def test_layernorm_stage_at_every_instantiation(C, g, N):
    """tests/test_vision_gpu.py test_layernorm_stage_on_a_known_input's method and bound: the launch with LayerNorm
    against float64 LayerNorm of the same launch's ln = None output e.  The inputs (ln_inputs) put a different offset on
    every 16-column tile and every wave's quarter of the row, and a product of about 3 in every column: a row sum that
    drops a tile, counts one twice or takes in a spare tile's accumulators leaves the bound at > 89 % of the row
    (tests/test_vision_widths_host.py).  The class row has no variance: its result is beta."""
    a = ln_inputs(g, N)
    ops = (a["img"], a["norm"], a["w"], a["cls"], a["pos"])
    e = launch(C, *ops)
    # e itself against the restatement: the FP32 sum may round to the other FP16 neighbour of the exact one (one ulp of
    # the product away), which the rounding of the sum with pos passes on within half an ulp of e on either side
    want_e, acc, _ = vision_ref.embed(*ops)
    e_err = np.abs(e.astype(np.float64) - want_e.astype(np.float64))
    e_tol = np.spacing(np.maximum(np.abs(e), np.abs(want_e))).astype(np.float64)
    e_tol[:, 1:] += np.spacing(np.abs(acc).astype(np.float16)).astype(np.float64)
    assert same(e[:, 0], want_e[:, 0]) and (e_err <= e_tol).all()
    got = launch(C, *ops, ln=(a["gamma"], a["beta"]), eps=EPS)
    y, tol = ln_tolerance(e, a["gamma"], a["beta"])
    err = np.abs(got.astype(np.float64) - y)
    print(f"LayerNorm stage g {g} N {N} (MAXT {maxt_of(N)}, nt {N // 64}): max err {err.max():.3e}, "
          f"max err / tol {(err / tol).max():.3f}")
    assert (err <= tol).all()
    assert np.ptp(e[:, 0].astype(np.float32)) == 0
    assert same(got[:, 0], np.broadcast_to(a["beta"], got[:, 0].shape).copy())


@pytest.mark.parametrize("with_ln", (False, True))
@pytest.mark.parametrize("pad", (4, 64))
@pytest.mark.parametrize("N", (1024, 832))
def test_output_pitch_above_n(C, N, pad, with_ln):
    """The C entry point with ldo = N + pad into a buffer of sentinels with one row to spare: the columns below N are
    clip_patch_embed's (ldo = N) bit for bit, every other element still the sentinel.  N = 1024 fills MAXT = 16;
    N = 832 leaves it three spare tiles per wave, 48 columns: inside the wider padding."""
    g, B, ldo = 2, 2, N + pad
    a = ln_inputs(g, N, B)
    rows = g * g + 1
    img, norm = t(a["img"]), t(np.asarray(a["norm"], np.float32))
    packed, cls, pos = C.clip_pack_patch_weight(t(a["w"])), t(a["cls"]), t(a["pos"])
    ln = (t(a["gamma"]), t(a["beta"])) if with_ln else (None, None)
    want = C.clip_patch_embed(img, norm, packed, cls, pos, *ln, EPS)
    out = torch.full((B * rows + 1, ldo), 7.0, dtype=torch.float16, device=DEV)
    code = C._lib.mixdq_clip_patch_embed_f16(img.data_ptr(), C.IMAGE_DTYPES[img.dtype], *img.stride(), norm.data_ptr(),
                                             packed.data_ptr(), cls.data_ptr(), pos.data_ptr(), rows, C._ptr(ln[0]),
                                             C._ptr(ln[1]), EPS, out.data_ptr(), ldo, B, 14 * g, N,
                                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == 0
    assert torch.equal(out[:-1, :N].reshape(B, rows, N).view(torch.int16), want.view(torch.int16))
    assert bool((out[:-1, N:] == 7.0).all()) and bool((out[-1] == 7.0).all())


@pytest.mark.parametrize("layout", ("contiguous", "channels_last"))
def test_largest_grid(C, layout):
    """g = 32, 448 px: 64 full blocks and the class block."""
    g, N, B = 32, 64, 1
    img, w, cls, pos = exact_inputs(g, N, B)
    want = vision_ref.embed(img, ONE, w, cls, pos)[0]
    got = launch(C, laid_out(t(img), layout), ONE, w, cls, pos)
    assert got.shape == (B, g * g + 1, N) and same(got, want)


@pytest.mark.parametrize("layout", ("contiguous", "channels_last"))
@pytest.mark.parametrize("norm", ("clip", "pm1"))
@pytest.mark.parametrize("dtype", (np.float16, np.float32))
def test_float_pixels_through_the_fma(C, dtype, norm, layout):
    """Float pixels k / 8 in 0 .. 255 with a, b that are not (1, 0); one tap per column, so out = f16(f16(fma(u, a, b))
    + pos).  The restatement's float64 u * a + b is exact for these values (tests/test_vision_widths_host.py), so its
    FP32 rounding is the fma's: equality of bits."""
    g, N = 4, 64
    px, nrm, w = fma_pixels(dtype), fma_norms()[norm], one_tap_filter(N)
    rng = np.random.default_rng(1)
    cls, pos = (rng.standard_normal(s).astype(np.float16) for s in ((N,), (g * g + 1, N)))
    want = vision_ref.embed(px, nrm, w, cls, pos)[0]
    got = launch(C, laid_out(t(px), layout), nrm, w, cls, pos)
    assert same(got, want)
