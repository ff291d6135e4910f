"""The resampling feature on the host: the tables of mixdq_amd/image.py against PIL and scipy, their invariants,
crop_region, the three new functions of include/mixdq_math.h -- compiled by the host compiler without contraction into a
stand-alone program -- against their numpy restatement (tests/resample_ref.py), the three entry points loaded on a
CPU-only box with every refusal of their argument checks, and Sampler.inpaint's new keywords."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, ALIGNMENT = 0, 1, 2
FILTER_NAMES = ("bilinear", "bicubic", "lanczos3")
f32 = np.float32

# (source (H, W), destination (H, W), box (x0, y0, x1, y1) or None)
PIL_CASES = [((37, 53), (48, 64), (5, 3, 41, 30)), ((64, 80), (16, 24), None), ((40, 40), (57, 13), (7.5, 2.25, 33, 39)),
             ((96, 96), (24, 24), None)]


def _tables(src_hw, dst_hw, box, name):
    from mixdq_amd.image import resample_table
    (Hs, Ws), (Hd, Wd) = src_hw, dst_hw
    x0, y0, x1, y1 = box if box is not None else (0, 0, Ws, Hs)
    xs, wx = resample_table(Ws, x0, x1, Wd, name)
    ys, wy = resample_table(Hs, y0, y1, Hd, name)
    return xs[None], wx[None], ys[None], wy[None]


@pytest.mark.parametrize("case", PIL_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}to{c[1][0]}x{c[1][1]}")
@pytest.mark.parametrize("name", FILTER_NAMES)
def test_tables_and_restatement_reproduce_pil(name, case):
    """resample_table + the FP32 restatement against PIL.Image.resize on mode-'F' images (PIL accumulates in double and
    stores float32 between its two passes), random 0..255 data: max |delta| <= 2e-4, about 6 FP32 ulp at 256 -- a wrong
    tap or start index moves results by more than 0.1.  Measured maxima over the four cases: bilinear 3.1e-5, bicubic
    4.6e-5, lanczos3 6.1e-5."""
    Image = pytest.importorskip("PIL.Image")
    src_hw, dst_hw, box = case
    rng = np.random.default_rng(src_hw[0] * 1000 + dst_hw[1])
    img = (rng.random(src_hw) * 255).astype(f32)
    flt = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos3": Image.LANCZOS}[name]
    want = np.asarray(Image.fromarray(img, "F").resize((dst_hw[1], dst_hw[0]), flt, box=box), dtype=f32)
    got = R.resample(img[None, None], *_tables(src_hw, dst_hw, box, name))[0, 0]
    delta = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{name} {case}: max |delta| = {delta:.3g}")
    assert got.shape == want.shape and delta <= 2e-4, delta


@pytest.mark.parametrize("n,sigma", [(37, 1), (53, 4), (9, 4), (64, 0.5)])
def test_gaussian_table_is_scipys_normalised_filter(n, sigma):
    ndi = pytest.importorskip("scipy.ndimage")
    from mixdq_amd.image import gaussian_table
    start, w = gaussian_table(n, sigma)
    radius = int(3 * sigma + 0.5)
    assert w.shape == (n, min(2 * radius + 1, n)) and w.dtype == f32 and start.dtype == np.int32
    # the float64 weights behind the table, rebuilt the same way, applied to a random vector
    rng = np.random.default_rng(n)
    v = rng.random(n)
    got = np.empty(n)
    for x in range(n):
        lo, hi = max(x - radius, 0), min(x + radius + 1, n)
        assert start[x] == lo
        d = np.arange(lo, hi, dtype=np.float64) - x
        k = np.exp(-(d * d) / (2.0 * sigma * sigma))
        k /= k.sum()
        assert np.array_equal(w[x, :hi - lo], k.astype(f32)) and not w[x, hi - lo:].any()
        got[x] = (k * v[lo:hi]).sum()
    want = (ndi.gaussian_filter1d(v, sigma, mode="constant", truncate=3)
            / ndi.gaussian_filter1d(np.ones(n), sigma, mode="constant", truncate=3))
    assert float(np.abs(got - want).max()) <= 1e-12


def _table_invariants(start, w, in_size):
    assert start.dtype == np.int32 and w.dtype == f32 and w.ndim == 2 and len(start) == len(w)
    assert (start >= 0).all()
    used = np.array([np.flatnonzero(r)[-1] + 1 for r in w])
    assert (start + used <= in_size).all()
    assert float(np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max()) <= 1e-6
    assert w.shape[1] >= used.max()           # (a filter's own zero can end a row: bilinear at 1:1 has taps 1, 0)


@pytest.mark.parametrize("name", FILTER_NAMES)
def test_resample_table_invariants(name):
    from mixdq_amd.image import resample_table
    for in_size, lo, hi, out in ((53, 5, 41, 64), (80, 0, 80, 24), (40, 7.5, 33, 13), (40, 2.25, 39, 57), (96, 0, 96, 24),
                                 (37, 0, 37, 37), (7, 0, 7, 1), (1, 0, 1, 5), (1024, 0, 1024, 512), (300, 299.5, 300, 3)):
        start, w = resample_table(in_size, lo, hi, out, name)
        assert len(start) == out
        _table_invariants(start, w, in_size)
    start, w = resample_table(37, 0, 37, 37, name)                  # 1:1 is the identity: the centre tap is 1.0f
    centre = np.take_along_axis(w, (np.arange(37) - start)[:, None], axis=1)[:, 0]
    assert np.array_equal(centre, np.ones(37, f32))
    rest = np.abs(w).sum(axis=1) - 1.0                               # (lanczos: sin(k pi) is 1e-16, not 0)
    assert (rest == 0).all() if name != "lanczos3" else (rest < 1e-15).all()
    start, w = resample_table(80, 0, 80, 20, "lanczos3")            # a 4x downscale: 24 taps
    assert w.shape[1] == 24
    with pytest.raises(RuntimeError, match="filter should be"):
        resample_table(8, 0, 8, 4, "nearest")
    with pytest.raises(RuntimeError, match="box"):
        resample_table(8, 3, 3, 4, name)
    with pytest.raises(RuntimeError, match="box"):
        resample_table(8, 0, 9, 4, name)
    with pytest.raises(RuntimeError, match="taps"):
        resample_table(4096, 0, 4096, 8, "lanczos3")


@pytest.mark.parametrize("n,sigma", [(37, 1), (53, 4), (9, 4), (64, 0.5), (1, 2.0)])
def test_gaussian_table_invariants(n, sigma):
    from mixdq_amd.image import gaussian_table
    _table_invariants(*gaussian_table(n, sigma), n)


def test_crop_region():
    from mixdq_amd.image import crop_region
    # hand-worked, 512x512 model (aspect 1), image 400 wide x 300 high
    hw, m = (300, 400), (512, 512)
    assert crop_region((100, 100, 150, 120), hw, m, 10) == (90, 75, 160, 145)     # 70x40 -> 70x70, centred
    assert crop_region((0, 100, 20, 200), hw, m, 0) == (0, 100, 100, 200)          # left border: shifted right
    assert crop_region((390, 100, 400, 200), hw, m, 0) == (300, 100, 400, 200)     # right border
    assert crop_region((100, 0, 200, 10), hw, m, 0) == (100, 0, 200, 100)          # top border
    assert crop_region((100, 295, 200, 300), hw, m, 0) == (100, 200, 200, 300)     # bottom border
    assert crop_region((10, 10, 20, 20), hw, m, 1000) == (0, 0, 400, 300)          # the pad reaches every border
    assert crop_region((0, 0, 400, 10), hw, m, 0) == (0, 0, 400, 300)              # 400 high does not fit: whole extent
    assert crop_region((5, 5, 5, 9), hw, m, 32) == (0, 0, 400, 300)                # an empty bbox
    assert crop_region((0, 0, 0, 0), hw, m, 32) == (0, 0, 400, 300)
    # a 3:2 model (Hm 256, Wm 384): 40 high -> 60 wide
    assert crop_region((100, 100, 110, 140), hw, (256, 384), 0) == (75, 100, 135, 140)
    rng = np.random.default_rng(5)
    for _ in range(2000):
        H, W = (int(v) for v in rng.integers(1, 500, 2))
        Hm, Wm = (8 * int(v) for v in rng.integers(1, 130, 2))
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        x1, y1 = int(rng.integers(x0 + 1, W + 1)), int(rng.integers(y0 + 1, H + 1))
        pad = int(rng.integers(0, 64))
        c = crop_region((x0, y0, x1, y1), (H, W), (Hm, Wm), pad)
        assert 0 <= c[0] <= x0 < x1 <= c[2] <= W and 0 <= c[1] <= y0 < y1 <= c[3] <= H          # inside, contains
        w, h = c[2] - c[0], c[3] - c[1]
        aspect = w == -(-h * Wm // Hm) or h == -(-w * Hm // Wm)
        assert aspect or (w == W and w * Hm < h * Wm) or (h == H and w * Hm > h * Wm), (c, H, W, Hm, Wm)
        assert crop_region(c, (H, W), (Hm, Wm), 0) == c                                         # idempotent


_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "mixdq_math.h"

/* spec IN OUT blend|round|tap.  blend: no input, the 256^3 results in (m, d, o) order; round: one FP32 value per
   result; tap: three FP32 values (acc, w, v) per FP32 result */
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 3;
  if (argv[3][0] == 'b') {
    static uint8_t buf[65536];
    for (int m = 0; m < 256; ++m) {
      for (int d = 0; d < 256; ++d)
        for (int o = 0; o < 256; ++o) buf[d * 256 + o] = mixdq_blend_u8((uint8_t)m, (uint8_t)d, (uint8_t)o);
      fwrite(buf, 1, sizeof buf, out);
    }
  } else if (argv[3][0] == 'r') {
    float v;
    while (fread(&v, 4, 1, in) == 1) {
      const uint8_t u = mixdq_round_u8(v);
      fwrite(&u, 1, 1, out);
    }
  } else {
    float t[3];
    while (fread(t, 4, 3, in) == 3) {
      const float r = mixdq_resample_tap(t[0], t[1], t[2]);
      fwrite(&r, 4, 1, out);
    }
  }
  fclose(in);
  return fclose(out) ? 4 : 0;
}
"""


@pytest.fixture(scope="module")
def spec_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample_spec")
    src, exe = d / "spec.c", d / "spec"
    src.write_text(_MAIN)
    subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src), "-lm"])

    def run(values, mode, dtype):
        fin, fout = d / f"{mode}.in", d / f"{mode}.out"
        np.ascontiguousarray(values, dtype=f32).tofile(fin)
        subprocess.check_call([str(exe), str(fin), str(fout), mode])
        return np.fromfile(fout, dtype=dtype)
    return run


def test_blend_u8_specification_on_all_triples(spec_program):
    """mixdq_blend_u8 == the restatement == rint of the exact quotient for all 256^3 (m, d, o): 255 is odd, so no
    quotient lies half way and the rounding mode does not matter."""
    got = spec_program(np.zeros(0), "blend", np.uint8).reshape(256, 256, 256)
    d, o = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for m in range(256):
        assert np.array_equal(got[m], R.blend_u8(m, d, o)), m
        exact = (m * d + (255 - m) * o) / 255.0
        assert np.array_equal(got[m], np.rint(exact).astype(np.uint8)), m
        assert (np.abs(exact - np.floor(exact) - 0.5) > 1e-3).all()             # never a tie
    assert np.array_equal(got[0], o) and np.array_equal(got[255], d)


def test_round_u8_specification_on_every_fp16_pattern_and_the_ties(spec_program):
    halves = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(f32)
    ties = np.arange(-2, 258, dtype=f32) + f32(0.5)
    near = np.concatenate([np.nextafter(ties, f32(-1e9)), np.nextafter(ties, f32(1e9))])
    v = np.concatenate([halves, ties, near, np.array([254.99998, 255.0, 255.00002, -0.0, 1e-45, 3e38, -3e38], f32)])
    got = spec_program(v, "round", np.uint8)
    assert np.array_equal(got, R.round_u8(v))
    nan = np.isnan(v)
    assert nan.sum() == 2046 and not got[nan].any()
    assert got[v == np.inf].tolist() == [255] and got[v == -np.inf].tolist() == [0]
    t = got[65536:65536 + len(ties)]
    want = np.clip(np.rint(ties.astype(np.float64)), 0, 255)                     # half to even: 0.5 -> 0, 1.5 -> 2
    assert np.array_equal(t, want.astype(np.uint8)) and t[2] == 0 and t[3] == 2 and t[4] == 2 and t[-1] == 255
    ok = ~nan & np.isfinite(v)
    assert np.array_equal(got[ok], np.clip(np.rint(v[ok].astype(np.float64)), 0, 255).astype(np.uint8))


def test_tap_specification_skips_zero_weights(spec_program):
    rng = np.random.default_rng(3)
    n = 4096
    t = np.empty((n, 3), dtype=f32)
    t[:, 0] = rng.standard_normal(n) * 100
    t[:, 1] = rng.standard_normal(n)
    t[:, 2] = rng.random(n) * 255
    t[:256, 1] = 0.0
    t[256:512, 1] = -0.0
    inf, nan = f32(np.inf), f32(np.nan)
    edge = np.array([[1.5, 0.0, nan], [1.5, -0.0, nan], [1.5, 0.0, inf], [-0.0, 0.0, -inf], [nan, 0.0, 1.0],
                     [1.5, 1e-45, 1.0], [1.5, 0.25, inf], [1.5, 0.25, nan], [0.0, -0.25, 0.0], [3e38, 3e38, 3e38],
                     [1.0, 0.1, 0.3], [16777216.0, 1.0, 1.0]], dtype=f32)
    t = np.concatenate([t, edge])
    got = spec_program(t, "tap", f32)
    want = R.tap(t[:, 0], t[:, 1], t[:, 2])
    both_nan = np.isnan(got) & np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[~both_nan], want.view(np.uint32)[~both_nan])
    zero = t[:, 1] == 0
    assert zero.sum() >= 516 and np.array_equal(got.view(np.uint32)[zero], t[zero, 0].view(np.uint32))   # acc itself
    assert both_nan.sum() == 2                                                   # the acc that is NaN, and 0.25 * NaN
    # fused: the product is not rounded on its own (1 + 2^-24-ish cases differ from mul-then-add somewhere)
    with np.errstate(over="ignore"):
        unfused = (t[:n, 1] * t[:n, 2] + t[:n, 0]).astype(f32)
    assert (unfused != got[:n]).any()


def _lib():
    from mixdq_amd.build import build
    return ctypes.CDLL(build())


def test_entry_points_are_declared_and_exported():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "mixdq_hip.h")).read()
    for name in ("mixdq_resample", "mixdq_resample_paste_u8", "mixdq_mask_bbox"):
        assert hasattr(lib, name), name
        assert f"int {name}(" in header, name
    for line in ("#define MIXDQ_RESAMPLE_SRC_VALUE 0", "#define MIXDQ_RESAMPLE_SRC_MASK 1",
                 "#define MIXDQ_RESAMPLE_DST_U8 0", "#define MIXDQ_RESAMPLE_DST_U8_UNIT 1",
                 "#define MIXDQ_RESAMPLE_DST_F32 2", "#define MIXDQ_PASTE_MASK_BINARY 0", "#define MIXDQ_PASTE_MASK_SOFT 1",
                 "#define MIXDQ_ABI_VERSION 3"):
        assert line in header
    lib.mixdq_abi_version.restype = ctypes.c_int
    assert lib.mixdq_abi_version() == 3
    math_h = open(os.path.join(ROOT, "include", "mixdq_math.h")).read()
    for fn in ("mixdq_resample_tap(", "mixdq_round_u8(", "mixdq_blend_u8("):
        assert fn in math_h
    from mixdq_amd.build import SOURCES
    assert "image.hip" in SOURCES


def test_resample_rejects_bad_arguments():
    """Never-dereferenced pointers: every call fails its checks on the host, before any launch."""
    lib = _lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    fn = lib.mixdq_resample
    fn.argtypes = [vp, i32] + [i64] * 4 + [i32, vp, i32, vp, vp, i32, vp, vp, i32] + [i32] * 7 + [vp]
    fn.restype = i32
    p = 0x1000

    def call(src=p, dtype=0, mode=0, dst=p, kind=0, xs=p, wx=p, Tx=4, ys=p, wy=p, Ty=4, Bt=1, B=2, C=3, Hs=16, Ws=24,
             Hd=8, Wd=8):
        return fn(src, dtype, C * Hs * Ws, Hs * Ws, Ws, 1, mode, dst, kind, xs, wx, Tx, ys, wy, Ty, Bt, B, C, Hs, Ws, Hd,
                  Wd, None)
    for name in ("src", "dst", "xs", "wx", "ys", "wy"):
        assert call(**{name: None}) == INVALID, name
    assert call(dtype=3) == INVALID and call(dtype=-1) == INVALID
    assert call(mode=2) == INVALID and call(mode=-1) == INVALID
    assert call(kind=3) == INVALID and call(kind=-1) == INVALID
    assert call(C=0) == INVALID and call(C=5) == INVALID
    assert call(Tx=0) == INVALID and call(Tx=257) == INVALID and call(Ty=0) == INVALID and call(Ty=257) == INVALID
    assert call(Bt=0) == INVALID and call(Bt=3) == INVALID and call(B=3, Bt=2) == INVALID
    assert call(B=-1) == INVALID and call(Hs=-1) == INVALID and call(Wd=-2) == INVALID and call(Hd=-2) == INVALID
    assert call(Hs=0) == INVALID and call(Ws=0) == INVALID                     # an output without a source
    assert call(src=p + 1, dtype=1) == ALIGNMENT and call(src=p + 2, dtype=2) == ALIGNMENT
    assert call(dst=p + 2, kind=2) == ALIGNMENT
    for name in ("xs", "wx", "ys", "wy"):
        assert call(**{name: p + 2}) == ALIGNMENT, name
    assert call(src=p + 1, dtype=1, C=0) == INVALID                              # INVALID is named before ALIGNMENT
    assert call(xs=p + 2, Tx=300) == INVALID
    # nothing to do: no pointer is looked at, nothing is launched ...
    nul = dict(src=None, dst=None, xs=None, wx=None, ys=None, wy=None)
    assert call(B=0, Bt=1, **nul) == OK and call(Hd=0, **nul) == OK and call(Wd=0, Hs=0, Ws=0, **nul) == OK
    assert call(B=0, Bt=0, **nul) == OK                                          # (Bt == B)
    # ... but the codes are still checked
    assert call(B=0, kind=7, **nul) == INVALID and call(Hd=0, mode=3, **nul) == INVALID
    assert call(Wd=0, dtype=5, **nul) == INVALID and call(B=0, Tx=0, **nul) == INVALID


def test_resample_paste_rejects_bad_arguments():
    lib = _lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    fn = lib.mixdq_resample_paste_u8
    fn.argtypes = ([vp] + [i64] * 4 + [i32, i32, vp, vp, i32] + [i64] * 3 + [i32, vp, vp, vp, i32, vp, vp, i32]
                   + [i32] * 6 + [vp])
    fn.restype = i32
    p = 0x1000

    def call(dec=p, out=p, mask=p, dtype=0, mode=0, win=p, xs=p, wx=p, Tx=4, ys=p, wy=p, Ty=4, Bt=2, Ht=8, Wt=8, B=2,
             H=32, W=40, Hm=16, Wm=16):
        return fn(dec, 4 * Hm * Wm, 1, 4 * Wm, 4, Hm, Wm, out, mask, dtype, H * W, W, 1, mode, win, xs, wx, Tx, ys, wy,
                  Ty, Bt, Ht, Wt, B, H, W, None)
    for name in ("dec", "out", "mask", "win", "xs", "wx", "ys", "wy"):
        assert call(**{name: None}) == INVALID, name
    assert call(dtype=3) == INVALID and call(dtype=-1) == INVALID
    assert call(mode=2) == INVALID and call(mode=-1) == INVALID
    assert call(mode=1, dtype=1) == INVALID and call(mode=1, dtype=2) == INVALID  # a soft mask is uint8
    assert call(Tx=0) == INVALID and call(Ty=257) == INVALID and call(Bt=3) == INVALID and call(Bt=0) == INVALID
    assert call(B=-1) == INVALID and call(H=-1) == INVALID and call(Wt=-1) == INVALID and call(Hm=-1) == INVALID
    assert call(Hm=0) == INVALID and call(Wm=0) == INVALID
    assert call(dec=p + 1) == ALIGNMENT
    assert call(mask=p + 1, dtype=1) == ALIGNMENT and call(mask=p + 2, dtype=2) == ALIGNMENT
    for name in ("win", "xs", "wx", "ys", "wy"):
        assert call(**{name: p + 2}) == ALIGNMENT, name
    assert call(dec=p + 1, mode=1, dtype=1) == INVALID                           # INVALID is named before ALIGNMENT
    nul = dict(dec=None, out=None, mask=None, win=None, xs=None, wx=None, ys=None, wy=None)
    assert call(B=0, Bt=1, **nul) == OK and call(Ht=0, **nul) == OK and call(Wt=0, **nul) == OK
    assert call(H=0, **nul) == OK and call(W=0, **nul) == OK
    assert call(B=0, Bt=1, mode=9, **nul) == INVALID and call(Ht=0, dtype=4, **nul) == INVALID


def test_mask_bbox_rejects_bad_arguments():
    lib = _lib()
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    fn = lib.mixdq_mask_bbox
    fn.argtypes = [vp, i32, i64, i64, i64, vp, i32, i32, i32, vp]
    fn.restype = i32
    p = 0x1000

    def call(mask=p, dtype=0, out=p, B=1, H=16, W=24):
        return fn(mask, dtype, H * W, W, 1, out, B, H, W, None)
    assert call(mask=None) == INVALID and call(out=None) == INVALID
    assert call(dtype=3) == INVALID and call(dtype=-1) == INVALID
    assert call(B=-1) == INVALID and call(H=-1) == INVALID and call(W=-1) == INVALID
    assert call(mask=p + 1, dtype=1) == ALIGNMENT and call(mask=p + 2, dtype=2) == ALIGNMENT and call(out=p + 2) == ALIGNMENT
    assert call(mask=p + 1, dtype=3) == INVALID
    assert call(mask=None, out=None, B=0) == OK and call(mask=None, out=None, H=0) == OK
    assert call(mask=None, out=None, W=0, dtype=2) == OK
    assert call(mask=None, out=None, B=0, dtype=5) == INVALID


def test_inpaint_keywords_default_to_the_old_behaviour():
    import torch
    from mixdq_amd import sampler as S
    sig = inspect.signature(S.Sampler.inpaint)
    want = {"crop": None, "crop_pad": 32, "mask_blur": 0.0, "resample": "lanczos3"}
    for name, default in want.items():
        par = sig.parameters[name]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default == default, name
    old = ["self", "enc", "dec", "image", "mask", "noise", "encoder_hidden_states", "added_cond_kwargs", "strength",
           "step_noise", "latent_noise", "mask_mode", "composite", "seed", "latent_seed"]
    assert list(sig.parameters)[:len(old)] == old and list(sig.parameters)[len(old):] == list(want)
    assert sig.parameters["composite"].default is False and sig.parameters["mask_mode"].default == "nearest"
    # the refusals of the crop path come before anything touches the VAE, the UNet or the GPU
    sm = S.Sampler(None, "euler", 4)
    noise = torch.zeros(1, 4, 8, 8)
    pixels = torch.zeros(1, 3, 90, 100, dtype=torch.uint8)
    mask = torch.zeros(1, 90, 100, dtype=torch.uint8)
    box = (10, 10, 60, 60)
    with pytest.raises(RuntimeError, match="image should be uint8"):
        sm.inpaint(None, None, pixels.float(), mask, noise, None, composite=True, crop=box)
    with pytest.raises(RuntimeError, match="image should be uint8"):
        sm.inpaint(None, None, pixels.half(), mask, noise, None, crop=box)
    with pytest.raises(RuntimeError, match="composite should be True"):
        sm.inpaint(None, None, pixels, mask, noise, None, crop=box)
    with pytest.raises(RuntimeError, match="composite should be True"):
        sm.inpaint(None, None, pixels, mask, noise, None, composite=False, crop="auto")
    with pytest.raises(RuntimeError, match="resample should be"):
        sm.inpaint(None, None, pixels, mask, noise, None, composite=True, crop=box, resample="nearest")
    with pytest.raises(RuntimeError, match="mask should have"):
        sm.inpaint(None, None, pixels, mask[:, :64], noise, None, composite=True, crop=box)
    with pytest.raises(RuntimeError, match="box"):
        sm.inpaint(None, None, pixels, mask, noise, None, composite=True, crop=(10, 10, 60, 95))
    with pytest.raises(RuntimeError, match="crop should be"):
        sm.inpaint(None, None, pixels, mask, noise, None, composite=True, crop="largest")
