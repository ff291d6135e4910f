"""The census of the capped-grid launches: one row per `grid_blocks(` call site of mixdq_amd/csrc, and per row the
CROSSING CASES -- calls with more work items than the capped grid has lanes, so that every lane runs its grid-stride
loop body a second time.

grid_blocks(items, per_cu) (csrc/common.h) caps a grid at kNumCU * per_cu workgroups of 256 lanes; below
cap_items(per_cu) = 256 * per_cu * 256 items `i += stride` is never executed, and a wrong stride, a `for` that is
really an `if` or an index recomputed from blockIdx inside the loop all pass.  A crossing case

  * has more items than cap_items(per_cu),
  * has an item count that is no multiple of it (the last trip is partial), and
  * where the kernel divides the item index by a width or a batch extent, makes that extent no power of two and puts
    a batch boundary inside the first trip.

Rows are of two kinds.  `new(...)` cases are run by tests/test_grid_caps_gpu.py (bit equality against a restatement that
shares no code with the kernel); `old(...)` cases name a test the suite already had, with its shape copied here as
constants and the source text (`needles`) that states it there.  tests/test_grid_caps_host.py drives BOTH kinds through
the stand-in runtime of tests/launch_trace.py and checks the launch (kernel instantiation, grid at the cap, items beyond
it), and compares the set of rows with the `grid_blocks(` calls it finds in the sources.

`python -m tests.grid_caps <environment name>` is that test's child process: it prints {case: [status, launches]}.

Imports without a GPU and without the built library.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mixdq_amd", "csrc")
NUM_CU, LANES = 256, 256                   # csrc/common.h kNumCU; every capped launch has 256-lane workgroups
U8, F16, F32 = 0, 1, 2                     # include/mixdq_hip.h MIXDQ_IMAGE_*
CTYPE = {U8: "unsigned char", F16: "__half", F32: "float"}
SHORT = {U8: "u8", F16: "f16", F32: "f32"}
ELEM = {U8: 1, F16: 2, F32: 4}
NP_DTYPE = {U8: np.uint8, F16: np.float16, F32: np.float32}
ENVIRONMENTS = {"default": {}, "geglu_arith": {"MIXDQ_GEGLU_TAB": "0"}}


def cap_blocks(per_cu):
    return NUM_CU * per_cu


def cap_items(per_cu):
    return cap_blocks(per_cu) * LANES


# ----------------------------------------------------------------------------------------------------- the rows
def new(name, symbols, args, test, entry=None, ptr_off=None, null=(), layout="dense", **more):
    """A crossing case of tests/test_grid_caps_gpu.py: `test`[`name`].  symbols: the capped launches of the call, in
    order, as '<kernel><template arguments>'; args: the scalar arguments of the entry point; ptr_off: {pointer
    argument: byte offset from a 16-byte boundary}; null: pointer arguments passed as NULL."""
    return dict(kind="new", name=name, symbols=_list(symbols), args=args, test=test, entry=entry,
                ptr_off=ptr_off or {}, null=tuple(null), layout=layout, arrays={}, env="default", **more)


def old(name, symbols, args, test, needles, where=None, entry=None, null=(), arrays=None, env="default"):
    """A crossing case an existing test runs: `test` ('file::test id'); needles: source text of `where` (default: the
    test's file) that states the shape copied into `args`."""
    return dict(kind="old", name=name, symbols=_list(symbols), args=args, test=test, needles=tuple(needles),
                where=where or test.split("::")[0], entry=entry, ptr_off={}, null=tuple(null), layout="dense",
                arrays=arrays or {}, env=env)


def _list(v):
    return [v] if isinstance(v, str) else list(v)


def site(file, kernels, per_cu, item, entry, items, cases, extents=None, batch_items=None, via=None):
    """file, kernels: the call site (`via`: the host function that holds the call, where the launch is elsewhere);
    item: what one work item is; items(args) -> the item count, from the shape alone; extents(args): what the kernel
    divides the item index by; batch_items(args): items per batch element (None: the kernel has no batch extent)."""
    for c in cases:
        c["entry"] = c["entry"] or entry
    return dict(file=file, kernels=tuple(kernels), per_cu=per_cu, item=item, entry=entry, items=items, cases=cases,
                extents=extents or (lambda a: ()), batch_items=batch_items, via=via)


def dense4(B, C, H, W):
    """Element strides of a dense NCHW tensor."""
    return (C * H * W, H * W, W, 1)


def chlast4(B, C, H, W):
    """... and of one in channels-last storage."""
    return (H * W * C, 1, W * C, C)


# the image-sized sites share one shape: 2 x 520 x 509 pixels = 529 360 (cap 524 288; image 0 ends at 264 680)
B_, H_, W_ = 2, 520, 509
PIXELS = B_ * H_ * W_
MASK_H, MASK_W = 8 * H_, 8 * W_                                   # mask_to_latent: 4160 x 4072 -> 520 x 509
NARROW_PAD = 8                                                     # the narrow view's backing rows: W + 8 elements
DIL_H, DIL_W = 1031, 1019                                          # mask growth: 2 x 1031 x 1019 = 2 101 178 (cap 2 097 152)


def _bhw(a):
    return a["B"] * a["H"] * a["W"]


def mask_strides(H, W, layout):
    """[B, H, W] mask: dense, or every second element of rows twice as long (the strided slice)."""
    return dict(mb=H * W, mh=W, mw=1) if layout == "dense" else dict(mb=2 * H * W, mh=2 * W, mw=2)


def composite_args(mask_dtype, layout="dense"):
    """dense: decoded and original NCHW.  strided: decoded channels-last, original columns 1 .. W of rows W + 3 long,
    the mask every second element."""
    if layout == "dense":
        d, o = dense4(B_, 3, H_, W_), dense4(B_, 3, H_, W_)
    else:
        d, o = chlast4(B_, 3, H_, W_), dense4(B_, 3, H_, W_ + 3)
    return dict(db=d[0], dc=d[1], dh=d[2], dw=d[3], ob=o[0], oc=o[1], oh=o[2], ow=o[3], mask_dtype=mask_dtype,
                B=B_, H=H_, W=W_, **mask_strides(H_, W_, layout))


def ingest_masked_args(dtype, mask_dtype, C=3, layout="dense"):
    s = dense4(B_, C, H_, W_) if layout == "dense" else chlast4(B_, C, H_, W_)
    return dict(dtype=dtype, sb=s[0], sc=s[1], sh=s[2], sw=s[3], mask_dtype=mask_dtype, B=B_, C=C, H=H_, W=W_,
                **mask_strides(H_, W_, layout))


def mask_to_latent_args(dtype, mode, narrow=False):
    """narrow: columns 1 .. W of rows W + 8 long -- the base one element off every vector alignment."""
    w = MASK_W + (NARROW_PAD if narrow else 0)
    return dict(dtype=dtype, sb=MASK_H * w, sh=w, sw=1, B=B_, H=MASK_H, W=MASK_W, mode=mode)


def dilate_args(dtype, radius, layout="dense"):
    m = mask_strides(DIL_H, DIL_W, layout)
    return dict(dtype=dtype, sb=m["mb"], sh=m["mh"], sw=m["mw"], B=2, H=DIL_H, W=DIL_W, radius=radius)


LINEAR = dict(M=1031, N=1020, K=20, group_rows=0, group_stride=0, group_offset=0, residual_row_div=1, flags=0)


def conv_args(pad):
    """58 x 57 outputs of a 3x3 conv, 4 -> 320 channels: 1 057 920 outputs (cap 1 048 576)."""
    return dict(N=1, H=58 + 2 - 2 * pad, W=57 + 2 - 2 * pad, C=4, K=320, R=3, S=3, stride=1, pad=pad, residual_row_div=1,
                flags=0)


def _conv_items(a):
    P = (a["H"] + 2 * a["pad"] - a["R"]) // a["stride"] + 1
    Q = (a["W"] + 2 * a["pad"] - a["S"]) // a["stride"] + 1
    return a["N"] * P * Q * a["K"]


def _conv_extents(a):
    Q = (a["W"] + 2 * a["pad"] - a["S"]) // a["stride"] + 1
    return (a["K"], Q)


def _step_args(n, rows, **more):
    up = lambda v, m: (v + m - 1) // m * m
    return dict(n=n, rows_per_image=rows, row_stride=up(n, 8) + 8, guidance=5.0, **more)


_N_STEP = 8 * (2048 * 256 + 37) + 5
_N_MASKED3 = 3 * (2048 * 256 * 8 // 3 + 50)
_DT = (U8, F16, F32)
_GPU = "tests/test_grid_caps_gpu.py"

SITES = [
    # ------------------------------------------------------------------------------------------ csrc/vae.hip
    site("vae.hip", ["composite_u8_kernel"], 8, "a pixel", "mixdq_composite_u8", _bhw,
         [new(f"mask_{SHORT[d]}", f"composite_u8_kernel<{CTYPE[d]}>", composite_args(d), "test_composite") for d in _DT]
         + [new("mask_u8_strided", "composite_u8_kernel<unsigned char>", composite_args(U8, "strided"),
                "test_composite", layout="strided")],
         extents=lambda a: (a["W"], a["H"]), batch_items=lambda a: a["H"] * a["W"]),
    site("vae.hip", ["image_to_nhwc8_masked_kernel"], 8, "a pixel", "mixdq_image_to_nhwc8_f16_masked", _bhw,
         [new(f"{SHORT[t]}_mask_{SHORT[m]}", f"image_to_nhwc8_masked_kernel<{CTYPE[t]}, {CTYPE[m]}>",
              ingest_masked_args(t, m), "test_ingest_masked") for t in _DT for m in _DT]
         + [new(f"u8_mask_u8_c{c}", "image_to_nhwc8_masked_kernel<unsigned char, unsigned char>",
                ingest_masked_args(U8, U8, C=c), "test_ingest_masked") for c in (1, 4)]
         + [new("f16_mask_f32_strided", "image_to_nhwc8_masked_kernel<__half, float>",
                ingest_masked_args(F16, F32, layout="strided"), "test_ingest_masked", layout="strided")],
         extents=lambda a: (a["W"], a["H"]), batch_items=lambda a: a["H"] * a["W"]),
    site("vae.hip", ["mask_to_latent_kernel"], 8, "a latent pixel (an 8x8 block of the mask)", "mixdq_mask_to_latent",
         lambda a: a["B"] * (a["H"] // 8) * (a["W"] // 8),
         [c for d in _DT for c in (
             new(f"{SHORT[d]}_nearest", f"mask_to_latent_kernel<{CTYPE[d]}, false, false>", mask_to_latent_args(d, 0),
                 "test_mask_to_latent"),
             new(f"{SHORT[d]}_any_wide", f"mask_to_latent_kernel<{CTYPE[d]}, true, true>", mask_to_latent_args(d, 1),
                 "test_mask_to_latent"),
             new(f"{SHORT[d]}_any_narrow", f"mask_to_latent_kernel<{CTYPE[d]}, true, false>",
                 mask_to_latent_args(d, 1, narrow=True), "test_mask_to_latent", ptr_off={"mask": ELEM[d]},
                 layout="narrow"))],
         extents=lambda a: (a["W"] // 8, a["H"] // 8), batch_items=lambda a: (a["H"] // 8) * (a["W"] // 8)),
    site("vae.hip", ["inpaint_cond_kernel"], 8, "a latent pixel", "mixdq_inpaint_cond_f16", lambda a: a["pixels"],
         [new("L4", "inpaint_cond_kernel<true>", dict(pixels=PIXELS, L=4), "test_inpaint_cond"),
          new("L4_offset", "inpaint_cond_kernel<false>", dict(pixels=PIXELS, L=4), "test_inpaint_cond",
              ptr_off={"zl": 4}),
          new("L3", "inpaint_cond_kernel<false>", dict(pixels=PIXELS, L=3), "test_inpaint_cond"),
          new("L7", "inpaint_cond_kernel<false>", dict(pixels=PIXELS, L=7), "test_inpaint_cond")]),
    site("vae.hip", ["ip2p_cond_kernel"], 8, "a latent pixel", "mixdq_ip2p_cond_f16",
         lambda a: a["B"] * a["pixels_per_image"],
         [new(f"rows{r}_L{L}", f"ip2p_cond_kernel<{r}, {'true' if L == 4 else 'false'}>",
              dict(B=B_, pixels_per_image=H_ * W_, L=L, rows=r, scale=0.18215), "test_ip2p_cond")
          for r in (1, 3) for L in (4, 3)]),
    site("vae.hip", ["image_to_nhwc8_kernel"], 8, "a pixel", "mixdq_image_to_nhwc8_f16", _bhw,
         [old("u8", "image_to_nhwc8_kernel<unsigned char>",
              dict(dtype=U8, B=1, C=3, H=8, W=2048 * 32 + 24, sb=3 * 8 * (2048 * 32 + 24), sc=8 * (2048 * 32 + 24),
                   sh=2048 * 32 + 24, sw=1),
              "tests/test_vae_enc_gpu.py::test_ingest_channel_counts_grid_stride_and_errors",
              ["(1, 3, 8, 2048 * 32 + 24)"])],
         extents=lambda a: (a["W"], a["H"])),
    site("vae.hip", ["vae_latent_kernel"], 8, "four latent channels of a pixel", "mixdq_vae_latent_sample",
         lambda a: a["pixels"] * (a["L"] // 4),
         [old("noise_L4", "vae_latent_kernel<true, true>", dict(pixels=2048 * 256 + 77, L=4, scaling_factor=0.18215),
              "tests/test_vae_enc_gpu.py::test_latent_sample_grid_stride_and_errors",
              ["n = 2048 * 256 + 77", "(1, 1, n, 8)", "0.18215"])]),
    # ---------------------------------------------------------------------------------------- csrc/image.hip
    site("image.hip", ["mask_dilate_rows_kernel", "mask_dilate_cols_kernel"], 32, "a pixel (both launches)",
         "mixdq_mask_dilate_u8", _bhw,
         [new(f"{SHORT[d]}_r2", [f"mask_dilate_rows_kernel<{CTYPE[d]}>", "mask_dilate_cols_kernel"], dilate_args(d, 2),
              "test_mask_dilate") for d in _DT]
         + [new("u8_r40", ["mask_dilate_rows_kernel<unsigned char>", "mask_dilate_cols_kernel"], dilate_args(U8, 40),
                "test_mask_dilate"),
            new("f32_r2_strided", ["mask_dilate_rows_kernel<float>", "mask_dilate_cols_kernel"],
                dilate_args(F32, 2, "strided"), "test_mask_dilate", layout="strided")],
         extents=lambda a: (a["W"], a["H"]), batch_items=lambda a: a["H"] * a["W"]),
    # ---------------------------------------------------------------------------------------- csrc/igemm.hip
    site("igemm.hip", ["igemm_generic_kernel"], 16, "an output", "mixdq_qlinear_w8a8_rows",
         lambda a: a["M"] * a["N"] if "M" in a else _conv_items(a),
         [new("linear_k20", "igemm_generic_kernel<false>", LINEAR, "test_igemm_generic_linear",
              null=["residual_f16_or_null"]),
          new("conv_c4_pad1", "igemm_generic_kernel<true>", conv_args(1), "test_igemm_generic_conv",
              entry="mixdq_qconv2d_w8a8_table", null=["residual_f16_or_null", "bias0_or_null"]),
          new("conv_c4_pad0", "igemm_generic_kernel<true>", conv_args(0), "test_igemm_generic_conv",
              entry="mixdq_qconv2d_w8a8_table", null=["residual_f16_or_null", "table_or_null"])],
         extents=lambda a: (a["N"],) if "M" in a else _conv_extents(a)),
    site("igemm.hip", ["f16_generic_kernel"], 16, "an output", "mixdq_conv2d_f16", _conv_items,
         [old("conv_c4_k256", "f16_generic_kernel<true, 0>",
              dict(N=1, H=64, W=72, C=4, K=256, R=3, S=3, stride=1, pad=1, residual_row_div=1, flags=0),
              "tests/test_f16_gpu.py::test_conv2d_f16_vs_fp32_reference[c4_k256_3x3_s1p1]",
              ["(1, 4, 64, 72, 256, 3, 1, 1, True)"], null=["residual_f16_or_null"])],
         extents=_conv_extents),
    site("igemm.hip", ["border_table_kernel"], 8, "a table entry", "mixdq_conv_border_table",
         lambda a: a["R"] * a["R"] * a["S"] * a["S"] * a["K"],
         [new("3x3_k6476", "border_table_kernel", dict(K=6476, R=3, S=3), "test_border_table")],
         extents=lambda a: (a["K"],)),
    site("igemm.hip", ["zp_propagate_kernel"], 8, "an output", "mixdq_conv_zero_point_propagate", _conv_items,
         [new("n2_29x31_k292", "zp_propagate_kernel", dict(N=2, H=29, W=31, K=292, R=3, S=3, stride=1, pad=1),
              "test_zp_propagate")],
         extents=lambda a: _conv_extents(a) + (a["H"],), batch_items=lambda a: _conv_items(a) // a["N"]),
    site("igemm.hip", ["gemm_f16_kernel"], 16, "an output", "mixdq_gemm_f16", lambda a: a["M"] * a["N"],
         [new("1031x1020x8", "gemm_f16_kernel", dict(M=1031, N=1020, K=8), "test_gemm_f16")],
         extents=lambda a: (a["N"],)),
    # ------------------------------------------------------------------------------------- csrc/quantize.hip
    site("quantize.hip", ["embed_tokens_kernel"], 8, "a 16-byte chunk of an output row", "mixdq_embed_tokens_f16",
         lambda a: a["B"] * a["T"] * (a["C"] // 8),
         [new("b401_t77_c136", "embed_tokens_kernel", dict(B=401, T=77, C=136, V=300), "test_embed_tokens")],
         extents=lambda a: (a["C"] // 8, a["T"]), batch_items=lambda a: a["T"] * (a["C"] // 8)),
    site("quantize.hip", ["quantize_dense_kernel"], 8, "an 8-element piece, plus one for the tail",
         "mixdq_quantize_f16_i8", lambda a: (a["_numel"] >> 3) + 1,
         [old("dense_deep", "quantize_dense_kernel<false, false>",
              dict(ndim=1, flags=0, _numel=8 * (4 * 524288 + 524288 // 2 + 3) + 5),
              "tests/test_quantize_routes_gpu.py::test_index_coded[dense_deep-8]",
              ["_DEEP = 8 * (4 * GRID_CAP_LANES + GRID_CAP_LANES // 2 + 3) + 5", '_case("dense_deep", (_DEEP,)'],
              where="tests/quantize_routes.py",
              arrays=dict(sizes=[8 * (4 * 524288 + 524288 // 2 + 3) + 5], x_strides=[1], out_strides=[1]))],
         via="plan_quantize"),
    site("quantize.hip", ["quantize_rows_kernel", "quantize_scalar_kernel"], 8,
         "an 8-element piece (rows) or an element (scalar)", "mixdq_quantize_f16_i8",
         lambda a: a["_numel"] >> 3 if a["_rows"] else a["_numel"],
         [old("rows_two_trips", "quantize_rows_kernel<false, false>",
              dict(ndim=2, flags=0, _numel=2200 * 2048, _rows=True),
              "tests/test_quantize_routes_gpu.py::test_index_coded[rows_two_trips-8]",
              ["(2, 1100, 2056)",
               '_case("rows_two_trips", _TT, lambda b: b[..., :2048], "rows", 2, (1, 1, 2200, 2048)'],
              where="tests/quantize_routes.py",
              arrays=dict(sizes=[2200, 2048], x_strides=[2056, 1], out_strides=[2048, 1])),
          old("scalar_two_trips", "quantize_scalar_kernel<false, false>",
              dict(ndim=2, flags=0, _numel=2200 * 2047, _rows=False),
              "tests/test_quantize_routes_gpu.py::test_index_coded[scalar_two_trips-8]",
              ['_case("scalar_two_trips", _TT, lambda b: b[..., :2047], "scalar", 2, (1, 1, 2200, 2047)'],
              where="tests/quantize_routes.py",
              arrays=dict(sizes=[2200, 2047], x_strides=[2056, 1], out_strides=[2047, 1]))],
         via="plan_quantize"),
    # ----------------------------------------------------------------------------------- csrc/fused_norm.hip
    # (1024, 5120) is 5 Mi outputs: by default the table kernel takes it (from 2 Mi on), whose grid is not capped.
    # The arithmetic kernel reaches its cap only under MIXDQ_GEGLU_TAB=0, in the child of the test named here.
    site("fused_norm.hip", ["geglu_quant_kernel"], 8, "an 8-element piece", "mixdq_geglu_quantize",
         lambda a: a["M"] * (a["D"] // 8),
         [old("1024x5120_tab0", "geglu_quant_kernel<false, false>", dict(M=1024, D=5120, flags=0),
              "tests/test_fused_gpu.py::test_geglu_table_variant_same_bits",
              ['@pytest.mark.parametrize("M,D", [(1024, 5120),', 'for flag in ("1", "0"):', "MIXDQ_GEGLU_TAB=flag",
               "test_geglu_quantize or"], env="geglu_arith")],
         extents=lambda a: (a["D"] // 8,)),
    # -------------------------------------------------------------------------------------- csrc/sampler.hip
    site("sampler.hip", ["sampler_step_kernel"], 8, "eight elements", "mixdq_sampler_step", lambda a: a["n"] >> 3,
         [old("rows2_plain", "sampler_step_kernel<2, 1, 0, 0>",
              _step_args(_N_STEP, 2, n_steps=20, noise_stride=_N_STEP + 7),
              "tests/test_sampler_gpu.py::test_step_kernel_grid_stride_and_twenty_steps",
              ["n = 8 * (2048 * 256 + 37) + 5", "_run_kernel_steps(C, s.coef, s.t_table, n, 2, False, 5.0"],
              null=["noise_or_null"]),
          old("rows2_2m", "sampler_step_kernel<2, 2, 0, 0>", _step_args(_N_STEP, 2, n_steps=4),
              "tests/test_multistep_gpu.py::test_step_2m_kernel_grid_stride",
              ["n = 8 * (2048 * 256 + 37) + 5", "_run_2m_steps(C, s, n, 2, 5.0"], entry="mixdq_sampler_step_2m"),
          old("rows2_masked4", "sampler_step_kernel<2, 1, 0, 1>",
              _step_args(_N_STEP - 1, 2, n_steps=4, noise_stride=_N_STEP + 3, channels=4),
              "tests/test_inpaint_gpu.py::test_masked_step_kernel_grid_stride",
              ["n = 8 * (2048 * 256 + 37) + 4", '_run_masked_steps(C, schedule("euler", 4), n, 4, 2, False, 5.0'],
              entry="mixdq_sampler_step_masked", null=["noise_or_null"]),
          old("rows1_noise_masked3", "sampler_step_kernel<1, 1, 1, 2>",
              _step_args(_N_MASKED3, 1, n_steps=4, noise_stride=_N_MASKED3 + 7, channels=3),
              "tests/test_inpaint_gpu.py::test_masked_step_kernel_grid_stride",
              ['_run_masked_steps(C, schedule("euler_ancestral", 4), 3 * (2048 * 256 * 8 // 3 + 50), 3, 1, True'],
              entry="mixdq_sampler_step_masked"),
          old("rows1_seeded", "sampler_step_kernel<1, 1, 2, 0>",
              dict(_step_args(_N_STEP - 5, 1, n_steps=2, n_image=_N_STEP - 5), row_stride=_N_STEP - 5, guidance=0.0),
              "tests/test_rng_gpu.py::test_step_rng_more_vectors_than_lanes",
              ["n = 8 * (NUM_CU * 8 * 256 + 37)", "kw = dict(seeds=sd) if k == \"rng\" else {}"],
              entry="mixdq_sampler_step_rng"),
          old("rows1_noise", "sampler_step_kernel<1, 1, 1, 0>",
              dict(_step_args(_N_STEP - 5, 1, n_steps=2, noise_stride=_N_STEP - 5), row_stride=_N_STEP - 5,
                   guidance=0.0),
              "tests/test_rng_gpu.py::test_step_rng_more_vectors_than_lanes",
              ["n = 8 * (NUM_CU * 8 * 256 + 37)", "None if k == \"rng\" else noise"])]),
    site("sampler.hip", ["randn_kernel"], 8, "four normals of one image", "mixdq_randn_f32",
         lambda a: a["B"] * ((a["n_image"] + 3) // 4),
         [old("vec", "randn_kernel<true>", dict(B=1, n_image=256 * 8 * 256 * 8 + 4 * 37, stream=0, step=0),
              "tests/test_rng_gpu.py::test_randn_grid_stride", ["(NUM_CU * 8 * 256 * 8 + 4 * 37, 1)"]),
          old("odd_two_images", "randn_kernel<false>",
              dict(B=2, n_image=(256 * 8 * 256 * 8 + 4 * 37) // 2 + 3, stream=0, step=0),
              "tests/test_rng_gpu.py::test_randn_grid_stride", ["((NUM_CU * 8 * 256 * 8 + 4 * 37) // 2 + 3, 2)"])],
         extents=lambda a: ((a["n_image"] + 3) // 4,),
         batch_items=lambda a: (a["n_image"] + 3) // 4 if a["B"] > 1 else None),
    # (the suite's exhaustive run over 2^24 values has 2^23 quads: sixteen WHOLE trips, so no partial last one)
    site("sampler.hip", ["normals_from_bits_kernel"], 8, "four words", "mixdq_rng_normals_from_bits",
         lambda a: a["n_quads"],
         [new("quads", "normals_from_bits_kernel", dict(n_quads=2048 * 256 + 37), "test_normals_from_bits")]),
]

CASES = [dict(c, per_cu=s["per_cu"], file=s["file"], items=s["items"](c["args"]), extents=tuple(s["extents"](c["args"])),
              batch_items=s["batch_items"](c["args"]) if s["batch_items"] else None) for s in SITES for c in s["cases"]]
NEW = [c for c in CASES if c["kind"] == "new"]


def case_key(c):
    return f"{c['test']}[{c['name']}]"


def by_test(test):
    """The new cases of one GPU test function, and their ids."""
    cases = [c for c in NEW if c["test"] == test]
    assert cases, test
    return dict(argvalues=cases, ids=[c["name"] for c in cases])


def entry_args(c):
    """The scalar arguments the entry point takes (the table's own notes, `_name`, left out)."""
    return {k: v for k, v in c["args"].items() if not k.startswith("_")}


# ----------------------------------------------------------------------------------------------- the census
_FUNCTION = re.compile(r"^(?!template|namespace|using|static const|#|//|\})[\w:<>\*&\" ]*?\b(\w+)\s*\([^;{]*$")


def census():
    """[(file, kernels launched or 'via:<host function>')] of every grid_blocks( call in csrc/*.hip and *.h apart from
    its definition.  The kernels of a call: the one named before it in its own statement, or every `<name>_kernel ...
    <<<v` of the rest of its function when the call initialises a variable v; a call whose function launches nothing
    (a planner) is named by that function."""
    out = []
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".h")):
            continue
        lines = open(os.path.join(CSRC, f)).read().split("\n")
        for n, line in enumerate(lines):
            for m in re.finditer(r"\bgrid_blocks\(", line):
                if re.match(r"\s*inline int grid_blocks\(", line):
                    continue
                before = re.findall(r"(\w+_kernel)\b", line[:m.start()])
                if before:
                    out.append((f, (before[-1],)))
                    continue
                var = re.search(r"(\w+)\s*=\s*$", line[:m.start()])
                assert var, (f, n + 1, line)
                end = next(i for i in range(n, len(lines)) if lines[i].startswith("}"))
                body = "\n".join(lines[n:end])
                kernels = re.findall(r"(\w+_kernel)\b(?:<[^;]*?>)?\s*<<<\s*" + var.group(1) + r"\b", body)
                if kernels:
                    out.append((f, tuple(dict.fromkeys(kernels))))
                    continue
                start = next(i for i in range(n, -1, -1) if _FUNCTION.match(lines[i]))
                out.append((f, "via:" + _FUNCTION.match(lines[start]).group(1)))
    return out


def table_census():
    return [(s["file"], "via:" + s["via"] if s["via"] else s["kernels"]) for s in SITES]


# ------------------------------------------------------------------------------------------ the generators
# Shared by the CPU checks and the GPU tests.  `xp` is numpy or torch: only arange-style index arithmetic.
def pattern(i, cap):
    """Set / clear runs over a flat item index: 37 set, 74 clear, with one set run and one clear run planted across
    item `cap` (the first item of the second trip): set on [cap - 61, cap + 53), clear on [cap + 53, cap + 200)."""
    base = (i // 37) % 3 == 0
    return (base | ((i >= cap - 61) & (i < cap + 53))) & ~((i >= cap + 53) & (i < cap + 200))


def second_pattern(i):
    """The decoy of mask_to_latent's blocks: runs of 5."""
    return (i // 5) % 2 == 0


def mask_values(set_, i, dtype, xp):
    """Mask elements for a set / clear decision, both sides of the binarisation's threshold within one step of it:
    uint8 set 128 + i % 100, clear i % 128; floats set 0.5 + (i % 4) / 4, clear (i % 4) / 8 - 0.0 .. 0.375."""
    if dtype == U8:
        return xp.where(set_, 128 + i % 100, i % 128)
    return xp.where(set_, 0.5 + (i % 4) * 0.25, (i % 4) * 0.125)


def dilate_seed(i, y, x, cap):
    """The set pixels of the mask-growth input: every 97th pixel inside alternate 128 x 128 tiles, and a run of nine
    across item `cap`."""
    return ((i % 97 == 0) & ((y // 128) % 2 == 0) & ((x // 128) % 2 == 0)) | ((i >= cap - 4) & (i < cap + 5))


def box_dilate(s, r):
    """numpy [B, H, W] bool -> bool: the (2r + 1)-square maximum clipped at each image's border, by two running
    sums (the CPU check's; the GPU test compares with F.max_pool2d and, at radius 2, tests/inpaint9_ref)."""
    def along(a, axis):
        n = a.shape[axis]
        c = np.concatenate([np.zeros_like(np.take(a, [0], axis)), np.cumsum(a, axis=axis)], axis=axis)
        hi = np.minimum(np.arange(n) + r + 1, n)
        lo = np.maximum(np.arange(n) - r, 0)
        return (np.take(c, hi, axis) - np.take(c, lo, axis)) > 0
    return along(along(s.astype(np.int32), 2).astype(np.int32), 1)


def image_code(i, c):
    """Image bytes: (7 * i + c) % 251 of the flat pixel index i and the channel c."""
    return (7 * i + c) % 251


def token_ids(row, V):
    """Token ids as a permutation code of the flat row index b * T + t: 211 is prime to the vocabulary sizes in use."""
    return (row * 211 + 7) % V


def latent_planting(j, cap):
    """What mask_to_latent's input holds per latent pixel j: (p, q, r, c) -- the block's pixel (0, 0) is set where p, its
    pixel (r, c) (1 <= r, c <= 7, moving with j) where q, every other pixel of the block is clear.  NEAREST reads p,
    ANY reads p | q."""
    return pattern(j, cap), second_pattern(j), j % 7 + 1, (j // 7) % 7 + 1


# ------------------------------------------------------------------------------------------ the trace child
def trace(env_name):
    """{case key: [status, [[demangled kernel, grid x, block x, dynamic LDS], ...]]} of every case of one environment,
    each entry point driven through tests/launch_trace.py's stand-in runtime (nothing runs; pointers are dummies)."""
    import ctypes
    from tests import launch_trace as lt
    t = lt.Tracer()
    plain = subprocess.run(["c++filt"], input="\n".join(t.kernels), capture_output=True, text=True,
                           check=True).stdout.split("\n")
    out = {}
    for c in CASES:
        if c["env"] != env_name:
            continue
        scal = entry_args(c)
        e = t.entry(c["entry"], **scal)
        a = dict(e.base)
        for name, values in c["arrays"].items():
            a[name] = t.host(ctypes.c_int64, list(values))
        for name, off in c["ptr_off"].items():
            a[name] = a[name] + off
        for name in c["null"]:
            assert name in a, (c["entry"], name)
            a[name] = None
        status = e.fn(*(a[n] for n, _ in e.args))
        launches = []
        for ev in t.events():
            if ev[0] == "L":
                k, grid, block, lds = ev[1:].split(":")
                launches.append([plain[int(k)], [int(g) for g in grid.split(",")], block, int(lds)])
        out[case_key(c)] = [status, launches]
    return out


def run_children():
    """trace() of every environment, each in a fresh process (the knobs are read once per process)."""
    from tests import launch_trace as lt
    lt.build_trace_lib()
    out = {}
    for name, knobs in ENVIRONMENTS.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("MIXDQ_") or k == "MIXDQ_TRACE_OBJ"}
        env.update(knobs)
        r = subprocess.run([sys.executable, "-m", "tests.grid_caps", name], cwd=ROOT, env=env, capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        out.update(json.loads(r.stdout))
    return out


if __name__ == "__main__":
    json.dump(trace(sys.argv[1]), sys.stdout)
