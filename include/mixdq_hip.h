/*
 * mixdq_hip.h -- C-ABI of libmixdq_hip.so, the MI355X (gfx950) implementation of the
 * MixDQ W8A8 operator stack (quantize -> INT8 GEMM / implicit-GEMM conv -> dequant epilogue).
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types, no libtorch link.
 * Every entry point cites the reference interface it replaces (paths relative to the
 * reference checkout, kernels/mixdq_extension/...).  The Python shim that turns these back into
 * the reference's `mixdq_extension._C` functions is mixdq_amd/_C.py; the binding a reference
 * maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions (same as the reference's pybind layer):
 *   - all pointers are DEVICE pointers unless stated otherwise; inputs are borrowed;
 *   - outputs are caller-allocated (the Python shim uses torch.empty so the caching allocator
 *     and graph capture keep working);
 *   - every call is an asynchronous launch on `stream` (a hipStream_t passed as void*);
 *     no host synchronisation, no allocation, scalars (scale_inv, zero_point) are read on the
 *     device  =>  safe under hipGraph capture;
 *   - return value: MIXDQ_OK (0) or an error code; the shim raises RuntimeError with
 *     mixdq_status_string(code) (reference: TORCH_CHECK -> RuntimeError).
 *   - no global mutable state that a result depends on: what the library keeps per process is a zero
 *     page, the GELU table (read-only once built: by the first GEMM+GEGLU call, or mixdq_gelu_table()),
 *     and one "already set up on this device" flag per kernel instantiation (the > 64 KiB LDS opt-in)
 *     and for that table.  Entry points may be called from several threads on different devices.
 */
#ifndef MIXDQ_HIP_H_
#define MIXDQ_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: round 1.  2: status codes 5..9 returned where 1 returned MIXDQ_ERR_UNSUPPORTED; structs and
 * entry points added since (grouped / GEGLU / attention launches, FP16 layers, producer fusions).
 * 3: mixdq_qlinear_w8a8_geglu takes its weight rows in value|gate groups of 16 (was 32) and N % 32.
 * Bumped whenever an existing entry point changes its signature, operand layout or error behaviour. */
#define MIXDQ_ABI_VERSION 3

typedef void* mixdq_stream_t; /* hipStream_t */

enum mixdq_status {
  MIXDQ_OK = 0,
  MIXDQ_ERR_INVALID_ARG = 1,     /* null pointer, negative size, ndim out of range ...            */
  MIXDQ_ERR_ALIGNMENT = 2,       /* "Int8 kernel with input or output alignment not to 4 is not
                                    supported." (qlinear.cc:131-134, qconv2d.cc:200-203)          */
  MIXDQ_ERR_UNSUPPORTED = 3,     /* dilation != 1 (op/qconv2d.py:120 "dilation has bugs")         */
  MIXDQ_ERR_LAUNCH = 4,          /* hipGetLastError() != hipSuccess ("CUTLASS kernel failed")    */
  /* codes 5.. have no reference counterpart: limits of entry points the reference does not have */
  MIXDQ_ERR_W4_SHAPE = 5,        /* MIXDQ_FLAG_W4: K % 32 != 0 (conv: C % 32) or an operand pointer
                                    not 16-byte aligned                                           */
  MIXDQ_ERR_GEGLU_SHAPE = 6,     /* mixdq_qlinear_w8a8_geglu: N % 32, K % 16 or pointer alignment */
  MIXDQ_ERR_PADDING = 7,         /* conv: padding >= kernel size (a window with no in-image tap)  */
  MIXDQ_ERR_ROWMAP_RESIDUAL = 8, /* output row map and residual in one call                       */
  MIXDQ_ERR_SHAPE = 9,           /* shape outside a fused kernel's range (head_dim != 64, GroupNorm
                                    geometry, LayerNorm width, tensor rank)                       */
  MIXDQ_ERR_W2_SHAPE = 10        /* MIXDQ_FLAG_W2: K % 64 != 0, an operand pointer not 16-byte
                                    aligned, or a forced tile W2 does not take (ids 42, 43, 44, 45,
                                    56: weight stage not whole 1-KiB pieces; 27)                  */
};

/* Bit flags accepted by the compute entry points. */
enum mixdq_flags {
  /* Epilogue / quantize rounding variant.  Default (0) = variant A: the
     multiply-add is one fused FMA (what nvcc -fmad=true makes of the reference's mul+add).
     MIXDQ_FLAG_UNFUSED = variant B: round after the multiply, then add.                          */
  MIXDQ_FLAG_UNFUSED = 1,
  /* The weight operand of mixdq_qlinear_w8a8_rows / mixdq_qconv2d_w8a8[_table] is PACKED signed
     4-bit ("nibble-planar per 8": byte j of each 4-byte group holds k[8g+j] in the high nibble and
     k[8g+4+j] in the low nibble, two's complement; [N, K/2] bytes, conv [K,R,S,C/2]).  Needs
     K % 32 == 0 (conv: C % 32 == 0).  No reference counterpart: the reference's 4-bit layers
     fall back to FP16 (nn/Linear.py:31,133-134); results equal the W8 path run on the unpacked
     values.  bias0 / scale are those of the unpacked integers.  A packed 3x3 / stride 1 / pad 1 conv
     in the LDS-halo kernel's range (C % 64 == 0; mixdq_conv_halo_select_flags != 0) runs on that
     kernel's W4 instantiations, forced ids 90 .. 93 and MIXDQ_FLAG_UPSAMPLE2X included. */
  MIXDQ_FLAG_W4 = 2,
  /* mixdq_qconv2d_w8a8_table only: X is [N, H/2, W/2, C] and the conv runs on its nearest-neighbour
     2x upsampling (H, W stay the conv's input size) -- Upsample2D's conv(interpolate(x, 2.0)) without
     the upsampled tensor (quantizing commutes with nearest upsampling: the INT8 values are the same).
     3x3 / stride 1 / pad 1 shapes of the LDS-halo kernel only (mixdq_conv_halo_select != 0), else
     MIXDQ_ERR_SHAPE.  No reference counterpart.
     mixdq_conv2d_f16 takes the flag too (same contract: X is [N, H/2, W/2, C], H and W stay the conv's input size;
     the gather of the MFMA tiles reads pixel (y >> 1, x >> 1) and tests (y, x) against H and W, so the result has
     the bits of the conv on the materialised upsampling): 3x3 / stride 1 / pad 1, H and W even, C % 8 == 0,
     K % 4 == 0 and 16-byte aligned operands (the MFMA tiles), else MIXDQ_ERR_SHAPE with nothing written. */
  MIXDQ_FLAG_UPSAMPLE2X = 4,
  /* mixdq_qlinear_f16in_w8a8 only: the FP16 operand's rows follow the output row map (see there). */
  MIXDQ_FLAG_A_ROWMAP = 8,
  /* The weight operand of mixdq_qlinear_w8a8[_rows] / _geglu / _attn / _grouped is PACKED signed 2-bit
     ("crumb-planar per 16": within every group of 16 consecutive k, byte j (0..3) of the group's dword
     holds k[16g+j] in bits 7:6, k[16g+4+j] in 5:4, k[16g+8+j] in 3:2 and k[16g+12+j] in 1:0, two's
     complement; [N, K/4] bytes).  Values in [-2, 1]; needs K % 64 == 0 (MIXDQ_ERR_W2_SHAPE otherwise).
     Results equal the W8 / W4 paths run on the unpacked values, bit for bit; bias0 / scale are those of
     the unpacked integers.  Linear only: conv, FP16, GEMM + LayerNorm and FP16-operand entry points
     refuse it (MIXDQ_ERR_UNSUPPORTED; mixdq_qlinear_f16in_w8a8 and the LayerNorm launch: MIXDQ_ERR_SHAPE,
     the caller then quantizes and runs the GEMM).  Together with MIXDQ_FLAG_W4: MIXDQ_ERR_INVALID_ARG.
     No reference counterpart: the reference stores its 2-bit layers as 4-bit (TODO in its loader). */
  MIXDQ_FLAG_W2 = 16,
  /* mixdq_attention_f16[_prefetch] only: a causal mask -- query row i attends to keys 0 .. i (a text encoder's
     self-attention).  Head width 64, tq == tkv <= 128, FP16 output (out_scale_inv == null) and bits 8..15 of flags 0 or
     1: the launch is the short-key kernel's (one geometry whatever the batch: a batch row has the bits of the
     sequence alone); anything else answers MIXDQ_ERR_SHAPE with nothing written.  Same arithmetic, in the same
     order, as the unmasked launch: a masked score is -inf before the row maximum is taken. */
  MIXDQ_FLAG_CAUSAL = 32,
  /* mixdq_linear_f16 only: an activation in the epilogue.  With h = f16(acc + bias) -- what the unflagged launch
     stores -- the launch stores f16(act(f32(h))), what a stock FP16 Linear followed by the activation computes:
       MIXDQ_FLAG_ACT_GELU        act = mixdq_geluf (erf form): the value of mixdq_gelu_table at h
       MIXDQ_FLAG_ACT_QUICK_GELU  act = mixdq_quick_geluf: x / (1 + exp(-(1.702 x)))     (include/mixdq_math.h)
     Both together, or either with a residual: MIXDQ_ERR_INVALID_ARG.  Every other entry point refuses them
     (MIXDQ_ERR_UNSUPPORTED). */
  MIXDQ_FLAG_ACT_GELU = 64,
  MIXDQ_FLAG_ACT_QUICK_GELU = 128,
  /* bits 8..15: force a kernel configuration id (tuning / tests); 0 = automatic */
  /* A 4-bit activation quantizer in slot i (i = 0, 1, 2: the i-th quantizer of a launch; entry points with one
     quantizer use slot 0): the INT8 operand is the int8 quantizer with a narrower clamp,
       q = clamp(rint(fma(f32(x), *scale_inv, *zero_point)), -128, -113)
     -- Path A's clamp(round(x / delta) + zp_u, 0, 15) shifted by -128, as zero_point is for 8 bits.  The GEMMs
     read such an operand unchanged (acc - bias0 = sum w (q - zp) holds for any clamp).  Honoured by
     mixdq_quantize_f16_i8, mixdq_layernorm_quantize (per slot), mixdq_geglu_quantize, mixdq_attention_f16[_prefetch]
     and mixdq_qlinear_w8a8_attn; every other entry point that quantizes refuses them (MIXDQ_ERR_UNSUPPORTED: the
     caller then asks for FP16 and quantizes in a launch of its own).  No reference counterpart: the reference's
     kernels cannot take a 4-bit activation and run such a layer in FP16 (nn/Linear.py:31,133-134). */
  MIXDQ_FLAG_A4_0 = 1 << 16,
  MIXDQ_FLAG_A4_1 = 1 << 17,
  MIXDQ_FLAG_A4_2 = 1 << 18,
  /* mixdq_conv2d_f16 only: the `pad` rows and columns of zeros lie BELOW and RIGHT of the image only (F.pad(x, (0,
     pad, 0, pad)) in front of an unpadded conv, without that tensor): P = (H + pad - R) / stride + 1, Q likewise,
     and output pixel (p, q) reads its window from (p * stride, q * stride).  3x3 / stride 2 / pad 1 is the conv of
     diffusers' Downsample2D as the VAE encoder uses it.  On the MFMA tiles and on the one-output-per-thread kernel,
     with or without a residual or a forced tile id; same bits as the conv on the padded tensor.  Together with
     MIXDQ_FLAG_UPSAMPLE2X, or pad >= R or pad >= S: MIXDQ_ERR_SHAPE, nothing written.  mixdq_qconv2d_w8a8[_table]
     refuse it (MIXDQ_ERR_UNSUPPORTED: their zero-point border table is built for symmetric padding).  No reference
     counterpart. */
  MIXDQ_FLAG_PAD_AFTER = 1 << 19
};
#define MIXDQ_FLAG_A4_ANY (MIXDQ_FLAG_A4_0 | MIXDQ_FLAG_A4_1 | MIXDQ_FLAG_A4_2)
#define MIXDQ_FLAG_ACT_ANY (MIXDQ_FLAG_ACT_GELU | MIXDQ_FLAG_ACT_QUICK_GELU)

const char* mixdq_status_string(int status);
int mixdq_abi_version(void);
/* sha256 (first 16 hex digits) over the kernel sources this library was built from (mixdq_amd/build.py writes it
 * at build time): lets a run say which sources the LOADED library carries -- the provenance check of bench.py's
 * counter columns -- whatever MIXDQ_HIP_LIB points at. */
const char* mixdq_build_csrc_sha16(void);

/* ---------------------------------------------------------------------------------------------
 * a1. FP16 -> INT8 per-tensor affine quantize.
 * Replaces: quantize_per_tensor_to_int8 / quantize_per_tensor_to_int8_vectorized
 *           (csrc/quant_dequant/quantize.cc:9-53, quantize_kernel.cu:10-48,
 *            quantize_kernel_vectorized.cu:29-95).  One kernel serves both names.
 *   q = (int8) clamp(rint(fma(f32(x), *scale_inv, *zero_point)), -128, 127)
 * `sizes`/`x_strides`/`out_strides` are HOST arrays of length ndim (1..8), strides in elements.
 * The reference reads x linearly and ignores strides (quantize_kernel.cu:20-25), which is only
 * right for dense inputs; this entry point implements the intended strided semantics.
 */
int mixdq_quantize_f16_i8(const void* x_f16, int8_t* out,
                          const int64_t* sizes, const int64_t* x_strides,
                          const int64_t* out_strides, int ndim,
                          const float* scale_inv, const float* zero_point,
                          int flags, mixdq_stream_t stream);
/* What mixdq_quantize_f16_i8 would launch for these sizes, strides and pointers: the answer of the host function
 * the launch itself calls (dimensions sorted by x stride, size-1 dimensions dropped, mergeable neighbours
 * collapsed; more than four left: MIXDQ_ERR_SHAPE).  No GPU needed; x_f16 / out are looked at for their alignment
 * only (16 / 8 bytes) and never dereferenced.  Returns the status the launch would return before launching; with
 * MIXDQ_OK the outputs (each may be null) hold
 *   *route            0 dense (linear on both sides, 8 elements a lane-step), 1 rows (inner run contiguous on both
 *                     sides, a multiple of 8, outer strides multiples of 8, aligned), 2 scalar (one element a
 *                     lane-step); -1: no element, nothing is launched
 *   *rank             dimensions left after the collapse (1..4; 0 with route -1)
 *   collapsed_sizes4  their sizes, slowest first, right-aligned in four entries (leading entries 1)
 *   *blocks           blocks of 256 lanes in the grid (at most 8 per CU; the kernels grid-stride beyond). */
int mixdq_quantize_f16_i8_route(const int64_t* sizes, const int64_t* x_strides,
                                const int64_t* out_strides, int ndim,
                                const void* x_f16, const void* out,
                                int* route, int* rank, int64_t* collapsed_sizes4, int* blocks);

/* ---------------------------------------------------------------------------------------------
 * a2. INT8 x INT8 -> INT32 GEMM with FP32 epilogue -> FP16.
 * Replaces: qlinear_w8_a8_ohalf (csrc/qlinear/qlinear.cc:13-137) and the four CUTLASS kernels
 *           cutlassGemm_{withBias,noBias}_{optimal,small}Alignment.cu.
 *   D[m,n] = f16( fma( (f32(sum_k A[m,k]*W[n,k]) - bias0[n]), scale[n], f32(bias[n]) ) )
 *            (no bias: f16((acc - bias0[n]) * scale[n]))
 * A: [M,K] row-major (lda = K), W: [N,K] row-major, D: [M,N] row-major (ldd = N).
 * Alignment: K % 4 == 0 and N % 4 == 0, else MIXDQ_ERR_ALIGNMENT (qlinear.cc:96-134).
 * The reference's unused arguments (weight_scale, input_scale, input_zero_point,
 * weight_sum_by_input_channels) stay in the Python signature and are not passed down.
 */
int mixdq_qlinear_w8a8(const int8_t* A, const int8_t* W,
                       const float* bias0, const float* scale,
                       const void* bias_f16_or_null, void* D_f16,
                       int64_t M, int N, int K,
                       int flags, mixdq_stream_t stream);

/* Same GEMM with two extensions (no reference counterpart; both keep results bit-identical to the
 * unfused sequence of reference ops + torch ops):
 *  - an output row map, used by QuantizedLinear's BOS path (nn/Linear.py:178-194) to write rows
 *    straight into the [B, T, N] result instead of torch.cat:
 *      D_row(m) = (m / group_rows) * group_stride + group_offset + (m % group_rows)
 *    (group_rows = T-1 = 76, group_stride = T = 77, group_offset = 1).  group_rows <= 0 = identity;
 *  - a residual added after the epilogue's FP16 rounding, exactly as a following torch half add:
 *      D[m,n] = f16( f32(f16(epilogue)) + f32(residual[(m / residual_row_div) * N + n]) )
 *    residual_row_div = 1: a full [M,N] residual (x + attn(x), x + ff(x)); = P*Q: one row per
 *    image (h + time_emb[:, :, None, None] after a conv).  Not combinable with a row map.
 */
int mixdq_qlinear_w8a8_rows(const int8_t* A, const int8_t* W,
                            const float* bias0, const float* scale,
                            const void* bias_f16_or_null, void* D_f16,
                            int64_t M, int N, int K,
                            int group_rows, int group_stride, int group_offset,
                            const void* residual_f16_or_null, int64_t residual_row_div,
                            int flags, mixdq_stream_t stream);

/* a1 + a2 in ONE launch: the GEMM quantizes its own activation operand ("A8 quant fused into INT8 GEMM").
 * Replaces the reference's pair of launches per layer -- quant_op(x, act_scales_inv, act_zero_points) followed
 * by qlinear (nn/Linear.py:162-176); 1x1 / pad-0 convs on NHWC rows too (nn/Conv2d.py:294-311) -- with results
 * bit-identical to mixdq_quantize_f16_i8 -> mixdq_qlinear_w8a8_rows:
 *   A_q[m,k] = (int8) clamp(rint(fma(f32(A[m * lda + k]), *act_scale_inv, *act_zero_point)), -128, 127)
 *   D        = the a2 epilogue over A_q (row map, residual and MIXDQ_FLAG_W4 / _UNFUSED as above).
 * A_f16: FP16, row m at element offset m * lda (lda >= K, lda % 8 == 0, 16-byte aligned base: a dense
 * [M, K] matrix, or a column slice x[:, c0:c0+K] of a wider row-major / NHWC tensor).  MIXDQ_FLAG_A_ROWMAP:
 * the operand's row m is row (m / group_rows) * group_stride + group_offset + m % group_rows of A_f16 --
 * the same map as the output's, i.e. the BOS slice x[:, 1:, :] of a [B, T, K] tensor read in place.
 * Range: K a multiple of the chosen tile's K depth (128; 64 on the 128x128 / 256x128 tiles), operands
 * 16-byte aligned, the FP16 operand below 4 GiB; MIXDQ_ERR_SHAPE otherwise (the caller then issues the
 * two launches).  mixdq_qlinear_f16in_supported() answers that question without launching. */
int mixdq_qlinear_f16in_w8a8(const void* A_f16, int64_t lda,
                             const float* act_scale_inv, const float* act_zero_point,
                             const int8_t* W, const float* bias0, const float* scale,
                             const void* bias_f16_or_null, void* D_f16,
                             int64_t M, int N, int K,
                             int group_rows, int group_stride, int group_offset,
                             const void* residual_f16_or_null, int64_t residual_row_div,
                             int flags, mixdq_stream_t stream);
/* 1 if mixdq_qlinear_f16in_w8a8 takes this problem (sizes only; pointers must still be 16-byte aligned),
 * else 0.  `rows_addressed`: rows of A_f16 the operand spans (M, or the mapped extent under a row map). */
int mixdq_qlinear_f16in_supported(int64_t M, int N, int K, int64_t lda, int64_t rows_addressed, int w4);
/* 1 if the one launch is expected to be cheaper than mixdq_quantize_f16_i8 + mixdq_qlinear_w8a8_rows for this
 * problem (a cost model fitted to MI355X measurements, csrc/igemm_aq.hip): every workgroup quantizes the rows of
 * its own tile, so wide layers at small M repeat the quantizer's arithmetic N / BN times and lose to the
 * stand-alone kernel.  mixdq_amd's modules fuse where this says 1 (MIXDQ_F16IN=1: wherever supported; 0: never). */
int mixdq_qlinear_f16in_preferred(int64_t M, int N, int K, int w4);
/* Configuration id (MIXDQ_IGEMM_CONFIGS) the automatic choice makes for such a launch; -1 = unsupported. */
int mixdq_qlinear_f16in_select_id(int64_t M, int N, int K, int w4);

/* ---------------------------------------------------------------------------------------------
 * a3 + a4. INT8 NHWC implicit-GEMM conv2d (cross-correlation) with the same epilogue, and the
 * activation zero-point propagation for padded convs.
 * Replaces: qconv2d_w8_a8_ohalf (csrc/qconv2d/qconv2d.cc:27-206), the eight CUTLASS conv
 *           kernels cutlassConv2d_*.cu, and activation_zero_point_propagate
 *           (csrc/qconv2d/conv_act_zero_point_propagate.cu:11-83).
 * X: [N,H,W,C] int8 (channels-last), Wt: [K,R,S,C] int8 (channels-last weight),
 * D: [N,P,Q,K] f16 (channels-last), P = (H + 2*pad - R)/stride + 1 (same for Q).
 *   pad == 0: bias0[K] required (per-channel);  wsum ignored.
 *   pad  > 0: wsum[K,R,S] f32 and *zero_point required; per output pixel
 *             bias0[n,p,q,k] = f32(sum over in-bounds taps of wsum[k,r,s]) * zp.
 *             The reference materialises that as an [N,P,Q,K] f32 tensor on every call; here a
 *             small table of tap-subset sums (mixdq_conv_border_table) is built into `workspace`
 *             on the same stream and the conv epilogue looks its border class up per pixel.
 * `workspace`: device buffer of at least mixdq_qconv2d_workspace_bytes(K,R,S,pad) bytes
 *             (may be null when that is 0).
 * dilation must be 1 (MIXDQ_ERR_UNSUPPORTED otherwise); C % 4 == 0 and K % 4 == 0.
 * Geometry: any R, S, stride and pad with pad < R and pad < S (MIXDQ_ERR_PADDING otherwise, nothing written:
 * every window must hold an image row and column -- a border class is a non-empty tap rectangle, and the table
 * rows of empty rectangles are never read).  mixdq_conv2d_f16 has no such limit (zero padding needs no class).
 *
 * Operand alignment, every entry point.  Operands are expected on 16-byte boundaries (FP16 bias vectors: 8).
 * An operand off its boundary, but on its own element's natural alignment, is handled as follows:
 *   mixdq_qlinear_w8a8[_rows], mixdq_qconv2d_w8a8[_table], mixdq_linear_f16, mixdq_conv2d_f16:
 *       the one-output-per-thread generic kernel runs -- same bits, MIXDQ_OK.  (A conv in the LDS-halo kernel's
 *       range falls through to it as well; a FORCED halo tile or MIXDQ_FLAG_UPSAMPLE2X then returns MIXDQ_ERR_SHAPE.)
 *   the same entries with MIXDQ_FLAG_W4 / MIXDQ_FLAG_W2:     MIXDQ_ERR_W4_SHAPE / MIXDQ_ERR_W2_SHAPE
 *   mixdq_qlinear_w8a8_geglu (output: 8 bytes):                MIXDQ_ERR_GEGLU_SHAPE
 *   mixdq_qlinear_w8a8_grouped (A; W4 / W2: the packed code):  MIXDQ_ERR_ALIGNMENT
 *   mixdq_qlinear_w8a8_attn, mixdq_qlinear_w8a8_ln, mixdq_attention_f16, mixdq_sampler_step:  MIXDQ_ERR_ALIGNMENT
 *   mixdq_qlinear_f16in_w8a8:                                  MIXDQ_ERR_SHAPE (the caller issues the two launches)
 * A refusing entry writes nothing.  tests/test_conv_geometry_gpu.py pins each line.
 */
size_t mixdq_qconv2d_workspace_bytes(int K, int R, int S, int pad);

int mixdq_qconv2d_w8a8(const int8_t* X_nhwc, const int8_t* Wt_krsc,
                       const float* scale,
                       const float* wsum_krs_or_null, const float* zero_point,
                       const float* bias0_or_null,
                       const void* bias_f16_or_null, void* D_nhwc_f16,
                       void* workspace,
                       int N, int H, int W, int C, int K, int R, int S,
                       int stride, int pad, int dilation,
                       int flags, mixdq_stream_t stream);

/* The two halves of the call above, for callers that cache the table per layer
 * (mixdq_amd.nn.QuantizedConv2d does: the table depends only on the weights). */
int mixdq_conv_border_table(const float* wsum_krs, float* table,
                            int K, int R, int S, mixdq_stream_t stream);

int mixdq_qconv2d_w8a8_table(const int8_t* X_nhwc, const int8_t* Wt_krsc,
                             const float* scale,
                             const float* table_or_null, const float* zero_point,
                             const float* bias0_or_null,
                             const void* bias_f16_or_null, void* D_nhwc_f16,
                             int N, int H, int W, int C, int K, int R, int S,
                             int stride, int pad,
                             const void* residual_f16_or_null, int64_t residual_row_div,
                             int flags, mixdq_stream_t stream);

/* Stand-alone restatement of the reference's materialised zero-point propagation
 * (conv_act_zero_point_propagate.cu:11-83): out[n,p,q,k] f32, NHWC.  Not on the fast path;
 * kept so the a4 row of the scope table has a directly comparable artefact. */
int mixdq_conv_zero_point_propagate(const float* wsum_krs, const float* zero_point,
                                    float* out_npqk,
                                    int N, int H, int W, int K, int R, int S,
                                    int stride, int pad, mixdq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * FP16 debug GEMM.  Replaces: qlinear_fp_reference (csrc/qlinear/qlinear.cc:140-204,
 * cutlassGemm_reference.cu:117-283).  D[M,N] = A[M,K] * B[K,N], B row-major [K,N]
 * (qlinear.cc:161), FP32 accumulate, FP16 out.  Not on the hot path.
 */
int mixdq_gemm_f16(const void* A_f16, const void* B_f16_kn, void* D_f16,
                   int64_t M, int N, int K, mixdq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Producer fusions (no reference counterpart: the reference runs stock
 * PyTorch FP16 ops followed by its quantize kernel).  Each keeps the rounding points of the unfused
 * sequence -- normalised value -> FP16, SiLU / GELU -> FP16, product -> FP16 -- and then applies the
 * a1 quantizer to that FP16 value.  Reduction orders are fixed and the transcendental steps are
 * include/mixdq_math.h, so the oracle reproduces them bit-for-bit.
 *
 * GroupNorm (+SiLU) + quantize on an NHWC tensor x [N, HW, C] (fp16), G groups, gamma/beta fp16 [C].
 * Writes int8 [N, HW, C] (if out_q != null) and/or the fp16 activation (if out_f16 != null).
 * Needs C % 8 == 0 and groups that an 8-channel run straddles at most once
 * (MIXDQ_ERR_SHAPE otherwise).  `workspace`: mixdq_groupnorm_workspace_bytes() bytes. */
size_t mixdq_groupnorm_workspace_bytes(int N, int64_t HW, int C, int G);
int mixdq_groupnorm_silu_quantize(const void* x_nhwc_f16, const void* gamma_f16,
                                  const void* beta_f16, float eps, int apply_silu,
                                  const float* scale_inv, const float* zero_point,
                                  int8_t* out_q_or_null, void* out_f16_or_null, void* workspace,
                                  int N, int64_t HW, int C, int G, int flags,
                                  mixdq_stream_t stream);

/* The same on a channel concatenation that is never made in memory (an up-block's
 * cat([hidden, skip], dim=1)): channels 0 .. C1-1 are read from x [N, HW, C1], the remaining C - C1
 * from x2 [N, HW, C - C1] (C1 % 8 == 0; C1 == C and x2 == null: one source).  Every output is what
 * mixdq_groupnorm_silu_quantize gives on the concatenated tensor. */
int mixdq_groupnorm_silu_quantize2(const void* x_nhwc_f16, int C1, const void* x2_nhwc_f16_or_null,
                                   const void* gamma_f16, const void* beta_f16, float eps,
                                   int apply_silu, const float* scale_inv, const float* zero_point,
                                   int8_t* out_q_or_null, void* out_f16_or_null, void* workspace,
                                   int N, int64_t HW, int C, int G, int flags,
                                   mixdq_stream_t stream);

/* ... and, from the same pass, the INPUT itself quantized (no normalisation): raw_q[i] (HOST arrays
 * of two device pointers; entry 0: source x, entry 1: source x2; null entries / null arrays: none)
 * receives mixdq_quantize_f16_i8(source i; raw_scale_inv[i], raw_zero_point[i]) in that source's own
 * [N, HW, Cs] layout -- the operand of a layer that reads the same activation as the norm (the ResNet
 * block's 1x1 conv_shortcut beside norm1; a split shortcut quantizes each half with its own
 * quantizer, nn/Conv2d.py:330-343). */
int mixdq_groupnorm_silu_quantize3(const void* x_nhwc_f16, int C1, const void* x2_nhwc_f16_or_null,
                                   const void* gamma_f16, const void* beta_f16, float eps,
                                   int apply_silu, const float* scale_inv, const float* zero_point,
                                   int8_t* out_q_or_null, void* out_f16_or_null,
                                   const float* const* raw_scale_inv,
                                   const float* const* raw_zero_point, int8_t* const* raw_q,
                                   void* workspace, int N, int64_t HW, int C, int G, int flags,
                                   mixdq_stream_t stream);

/* LayerNorm over the last dimension of x [M, C] (fp16) + up to three quantizers of the same
 * normalised FP16 value (to_q / to_k / to_v have their own activation scales).  HOST arrays of
 * n_out device pointers.  C % 16 == 0, C <= 2048 (MIXDQ_ERR_SHAPE otherwise).  Row statistics in the
 * tiling-independent order of oracle/mixdq_oracle.c (per-16-column partials, Chan's combination), so that
 * mixdq_qlinear_w8a8_ln -- the same LayerNorm in the epilogue of the GEMM that produces x -- gives the same bits. */
int mixdq_layernorm_quantize(const void* x_f16, const void* gamma_f16, const void* beta_f16,
                             float eps, int64_t M, int C, int n_out,
                             const float* const* scale_inv, const float* const* zero_point,
                             int8_t* const* out_q, void* out_f16_or_null, int flags,
                             mixdq_stream_t stream);

/* a2 + residual + LayerNorm + quantize in ONE launch: the GEMM of mixdq_qlinear_w8a8_rows (bias, residual as
 * there; no row map) whose output rows D [M, N] are ALSO normalised over their N columns and quantized for up to
 * three consumers, exactly as mixdq_layernorm_quantize(D, ...) would do in a second launch:
 *   out_q[i][m, n] = quantize_i( f16( fma((D[m,n] - mean_m) * rstd_m, gamma[n], beta[n]) ) ),  out_f16 = that FP16.
 * A column tile of 80 columns is exactly one unit of the LayerNorm's reduction order (oracle/mixdq_oracle.c):
 * every tile publishes ONE 16-byte record per row -- {sum, centred sum of squares, launch tag} -- into
 * `workspace` with a write-through store, polls the N / 80 records of each of its rows until they carry this
 * launch's tag, combines them and normalises the columns it still holds in LDS; the bits equal the two-launch
 * chain.  Range: N = 1280 or 640 (N / 80 a power of two <= 16 that equals the LayerNorm's unit count),
 * K % 128 == 0, and the whole launch resident at once -- at most one 64 x 80 (or 128 x 80) tile per CU:
 * M <= 1024 at N = 1280 (2048 on 128-row tiles), M <= 4096 at N = 640 -- MIXDQ_ERR_SHAPE otherwise
 * (mixdq_qlinear_ln_select_id() < 0; the caller then issues the two launches).
 * `workspace`: mixdq_qlinear_ln_workspace_bytes(M, N) bytes, 16-byte aligned, ZERO before the first use (its
 * first page holds a launch counter that tags the records: a launch of any shape may follow on the same
 * buffer).  One launch at a time per workspace (launches of one stream are) AND per device: the tiles of a row
 * block wait for each other, so the whole grid must be resident at once -- the entry point checks the grid against
 * the device's real CU count and the runtime's occupancy answer (MIXDQ_ERR_SHAPE if it does not fit), but two such
 * launches on DIFFERENT streams of one device can each hold CUs the other needs: do not run them concurrently.  A
 * workgroup that gives up waiting (bounded spin) writes its rows as NaN and sets a sticky error word in the
 * workspace; mixdq_qlinear_ln_status() reads it (0 = every launch on this workspace found all its records).
 * No reference counterpart (stock nn.LayerNorm + quant_op, nn/Linear.py:162-164). */
size_t mixdq_qlinear_ln_workspace_bytes(int64_t M, int N);
int mixdq_qlinear_ln_select_id(int64_t M, int N, int K);   /* tile id (44, 45, 56) or -1 = not supported */
int mixdq_qlinear_ln_status(const void* workspace, int* status, mixdq_stream_t stream);   /* blocking; not in a capture */
int mixdq_qlinear_w8a8_ln(const int8_t* A, const int8_t* W, const float* bias0, const float* scale,
                          const void* bias_f16_or_null, void* D_f16, int64_t M, int N, int K,
                          const void* residual_f16_or_null, int64_t residual_row_div,
                          const void* gamma_f16, const void* beta_f16, float eps, int n_out,
                          const float* const* scale_inv, const float* const* zero_point,
                          int8_t* const* out_q, void* out_f16_or_null, void* workspace,
                          int flags, mixdq_stream_t stream);

/* GEGLU + quantize: h [M, 2D] fp16 (ff.net.0.proj output) -> fp16(h[:, :D] * fp16(gelu(h[:, D:])))
 * -> int8 [M, D] and/or fp16 [M, D].  D % 8 == 0. */
int mixdq_geglu_quantize(const void* h_f16, int64_t M, int D,
                         const float* scale_inv, const float* zero_point,
                         int8_t* out_q_or_null, void* out_f16_or_null, int flags,
                         mixdq_stream_t stream);

/* to_q + cross-attention in ONE launch: the INT8 GEMM of attn2.to_q (no bias) whose fp16 result --
 * 64 query rows x two heads per workgroup -- never leaves the chip: it is multiplied against the
 * (at most 128) keys / values of those heads with the arithmetic of mixdq_attention_f16, and the
 * attention output is written as to_out.0's INT8 operand (out_scale_inv given) or as fp16.
 * Bit-identical to mixdq_qlinear_w8a8 followed by mixdq_attention_f16.  No reference counterpart.
 * A [M, K] int8 (M = images x rows_per_image, rows_per_image % 64 == 0), W [N, K] (N % 128 == 0,
 * heads = N / 64, K % 128 == 0), k / v fp16 [images, tkv, N] with the given strides in elements
 * (multiples of 8; column slices of a packed k|v projection are fine), tkv <= 128. */
int mixdq_qlinear_w8a8_attn(const int8_t* A, const int8_t* W, const float* bias0, const float* scale,
                            const void* k_f16, const void* v_f16, void* out, int64_t M, int N, int K,
                            int rows_per_image, int tkv, int64_t k_batch_stride, int k_row_stride,
                            int64_t v_batch_stride, int v_row_stride, float softmax_scale,
                            const float* out_scale_inv_or_null, const float* out_zero_point_or_null,
                            int flags, mixdq_stream_t stream);

/* Grouped form of mixdq_qlinear_w8a8_rows: `ngroups` independent Linears that read the SAME int8
 * activations A [M, K] -- the 70 cross-attention k|v projections of the text embeddings, the 22
 * time-embedding projections -- in ONE launch (gridDim.y = member).  No reference counterpart (it
 * launches one GEMM per layer); every member's outputs are bit-identical to its own launch.
 * `groups_device`: DEVICE array of members; N may differ per member (max_N = the largest).  The
 * row map is shared.  K % 16 == 0 (W4: % 32) and N % 4 == 0. */
typedef struct mixdq_gemm_group {
  const int8_t* W;               /* [N, K] (MIXDQ_FLAG_W4: [N, K/2], MIXDQ_FLAG_W2: [N, K/4] packed) */
  const float* bias0;            /* [N] */
  const float* scale;            /* [N] */
  const void* bias_f16_or_null;  /* [N] */
  void* D_f16;                   /* output base */
  int32_t N;
  int32_t reserved;
} mixdq_gemm_group;
int mixdq_qlinear_w8a8_grouped(const int8_t* A, const mixdq_gemm_group* groups_device, int ngroups,
                               int64_t M, int max_N, int K, int group_rows, int group_stride,
                               int group_offset, int flags, mixdq_stream_t stream);

/* ff.net.0.proj + GEGLU + quantize in one launch: the GEMM of mixdq_qlinear_w8a8 whose N = 2D
 * output columns arrive as value|gate groups of 16 ([v 0..15 | g 0..15 | v 16..31 | g 16..31 ...]:
 * the caller stores W, bias0, scale and bias with rows in that order -- then every 32-column MFMA
 * tile holds the value and the gate of 16 outputs, in the same lanes), reduced in the epilogue to
 * out[m, d] = sat8(rint(y * scale_inv + zero_point)), y = f16(f16(v) * f16(gelu(f16(g)))) -- every
 * rounding point of GEMM -> fp16 -> mixdq_geglu_quantize is kept, so the int8 [M, D] result is
 * bit-identical to that two-launch chain (diffusers GEGLU: hidden, gate = proj(x).chunk(2);
 * hidden * gelu(gate)).  N % 32 == 0, K % 16 == 0 (MIXDQ_ERR_GEGLU_SHAPE otherwise). */
int mixdq_qlinear_w8a8_geglu(const int8_t* A, const int8_t* W_interleaved, const float* bias0,
                             const float* scale, const void* bias_f16_or_null, int8_t* out_i8,
                             int64_t M, int N, int K, const float* out_scale_inv,
                             const float* out_zero_point, int flags, mixdq_stream_t stream);

/* FP16 attention core, head_dim D = 64, 40, 80, 160 or 512 (MIXDQ_ERR_SHAPE otherwise).
 * D = 512 (the VAE decoder's single head; any `heads`): FP16 output only -- out_scale_inv != null is MIXDQ_ERR_SHAPE --
 * one launch geometry (32 query rows per workgroup, D split over its four waves: csrc/attention.hip
 * attn_512_kernel), so bits 8..15 of flags must be 0 (MIXDQ_ERR_SHAPE otherwise); any tq / tkv; a prefetch payload
 * is ignored.
 * 40 / 80 / 160: SD 1.5's heads --
 * forms 4 and 2 are one kernel, form 1 its short-key sibling for tkv <= 128, which is what a launch with so few keys
 * gets by default (MIXDQ_ATTN_HD_SHORT=0 in the environment: forms 4 / 2 there too, for A/B runs); all forms give the
 * same bits; a payload of mixdq_attention_f16_prefetch is ignored at these widths):
 * out[b, t, h*D + d] = softmax_k(q . k * softmax_scale) v, per
 * head h.  The reference keeps these matmuls in FP16 (quant_block.py:630-637: get_attention_scores
 * + torch.bmm; diffusers' AttnProcessor at run time) — only to_q/to_k/to_v/to_out.0 are quantized
 * Linears — so this is a floating-point op with a tolerance oracle, not an integer one.
 * q [batch, tq, heads*D], k/v [batch, tkv, heads*D] fp16 with arbitrary batch/row strides in
 * ELEMENTS (multiples of 8; column slices of a fused q|k|v projection are fine).  Softmax in FP32,
 * P rounded to FP16 for the second product, output rounded to FP16.
 * out: fp16 rows (out_scale_inv == null), or — fused producer of to_out.0's INT8 operand — int8
 * rows q = sat8(rint(f16_out * scale_inv + zero_point)) (same arithmetic as mixdq_quantize_f16_i8).
 * flags: MIXDQ_FLAG_UNFUSED selects the unfused quantize variant; bits 8..15 force the workgroup
 * shape (4 = 128 query rows, 2 = 64; 1 = the short-key kernel, at every width: MIXDQ_ERR_SHAPE when tkv > 128);
 * MIXDQ_FLAG_CAUSAL: see the flag. */
int mixdq_attention_f16(const void* q_f16, const void* k_f16, const void* v_f16, void* out,
                        int batch, int heads, int head_dim, int tq, int tkv,
                        int64_t q_batch_stride, int64_t q_row_stride,
                        int64_t k_batch_stride, int64_t k_row_stride,
                        int64_t v_batch_stride, int64_t v_row_stride,
                        int64_t out_batch_stride, int64_t out_row_stride,
                        float softmax_scale, const float* out_scale_inv_or_null,
                        const float* out_zero_point_or_null, int flags, mixdq_stream_t stream);

/* mixdq_attention_f16 with a PREFETCH payload: beside the attention workgroups the launch carries
 * workgroups that do nothing but read the `n_prefetch` (<= 16) given byte ranges (HOST arrays of device
 * pointers / sizes) -- the INT8 weights of the layers that FOLLOW this attention in the network.  At
 * batch 1 a 1024-token self-attention occupies 62 % of the SIMDs for ~17 us and leaves HBM idle, while
 * every GEMM behind it streams weights that were last touched a step ago (2.6 GB per step: nothing
 * survives in the 256 MB Infinity Cache); read here, they are served from that cache when their GEMM
 * runs.  The payload has no effect on any result.  No reference counterpart.
 * Ranges may be null / empty; the attention itself is mixdq_attention_f16's, bit for bit.  Launches on
 * the short-key kernel (tkv <= 128) ignore the payload. */
int mixdq_attention_f16_prefetch(const void* q_f16, const void* k_f16, const void* v_f16, void* out,
                                 int batch, int heads, int head_dim, int tq, int tkv,
                                 int64_t q_batch_stride, int64_t q_row_stride,
                                 int64_t k_batch_stride, int64_t k_row_stride,
                                 int64_t v_batch_stride, int64_t v_row_stride,
                                 int64_t out_batch_stride, int64_t out_row_stride,
                                 float softmax_scale, const float* out_scale_inv_or_null,
                                 const float* out_zero_point_or_null,
                                 const void* const* prefetch_ptrs, const int64_t* prefetch_bytes,
                                 int n_prefetch, int flags, mixdq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * FP16 layers.  Replaces the reference's FP fallback for layers without an activation quantizer
 * or with unsupported weight bits -- F.linear / F.conv2d on the FP16 weight (nn/Linear.py:155-156,
 * nn/Conv2d.py:306-309), i.e. cuBLAS / cuDNN there -- with the same LDS-DMA / MFMA kernel family
 * on FP16 operands (v_mfma_f32_32x32x16_f16, FP32 accumulation), so the captured step contains no
 * vendor-library kernel.  Floating point: a tolerance oracle (FP32 reference), not bit parity.
 *   D[m,n] = f16( sum_k f32(A[m,k]) * f32(W[n,k]) + f32(bias[n]) )  [+ residual, as above]
 * A [M,K], W [N,K], D [M,N] row-major fp16; conv: X [N,H,W,C], Wt [K,R,S,C], D [N,P,Q,K].
 * K % 8 == 0 (conv: C % 8 == 0) and N % 4 == 0 run on MFMA tiles, anything else (conv_in: C = 4)
 * on a one-output-per-thread kernel.  flags: bits 8..15 force a tile configuration; mixdq_conv2d_f16 also takes
 * MIXDQ_FLAG_UPSAMPLE2X (see the flag: the conv of Upsample2D without the upsampled tensor) and MIXDQ_FLAG_PAD_AFTER
 * (see the flag: padding below and right only, the conv of Downsample2D), mixdq_linear_f16
 * MIXDQ_FLAG_ACT_GELU / MIXDQ_FLAG_ACT_QUICK_GELU (see the flags: the activation of an MLP's first layer, applied to
 * the rounded FP16 value where the tile is stored -- the same on every tile configuration and on the
 * one-output-per-thread kernel). */
int mixdq_linear_f16(const void* A_f16, const void* W_f16, const void* bias_f16_or_null,
                     void* D_f16, int64_t M, int N, int K, const void* residual_f16_or_null,
                     int64_t residual_row_div, int flags, mixdq_stream_t stream);
int mixdq_conv2d_f16(const void* X_f16, const void* Wt_f16, const void* bias_f16_or_null,
                     void* D_f16, int N, int H, int W, int C, int K, int R, int S, int stride,
                     int pad, const void* residual_f16_or_null, int64_t residual_row_div,
                     int flags, mixdq_stream_t stream);

/* Token + position embedding of a text encoder:
 *   out[b, t, :] = f16_rn(f32(tok[ids[b, t]]) + f32(pos[t]))       ids int32 [B, T], tok fp16 [V, C], pos fp16 [>= T, C]
 * An id outside [0, V) is CLAMPED into the range (ids < 0 read row 0, ids >= V row V - 1): the kernel cannot report
 * an error, and a caller that wants to stay asynchronous cannot look at the ids.  C % 8 == 0 and 16-byte aligned
 * tok / pos / out (16-byte vector loads and stores): MIXDQ_ERR_ALIGNMENT otherwise; null pointers, negative sizes,
 * V < 1: MIXDQ_ERR_INVALID_ARG.  B * T == 0 writes nothing.  No reference counterpart (the reference reaches the
 * text encoders through diffusers' pipeline). */
int mixdq_embed_tokens_f16(const int32_t* ids, const void* tok_f16, const void* pos_f16, void* out_f16, int B, int T,
                           int C, int V, mixdq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * VAE encoder ends (csrc/vae.hip).  No reference counterpart (the reference reaches the VAE through diffusers'
 * pipeline).
 *
 * mixdq_image_to_nhwc8_f16: the encoder's ingest.  img: [B, C, H, W] of uint8 (dtype 0), FP16 (1) or FP32 (2),
 * element (b, c, y, x) at img + (b * sb + c * sc + y * sh + x * sw) ELEMENTS (NCHW and NHWC sources alike);
 * out: FP16 [B, H, W, 8], one 16-byte store per pixel, channels C..7 zero.
 *   uint8:  f16_rn(f32(u) * (2/255: 0x3C008081) - 1.0f)     two FP32 roundings, never contracted: u / 127.5 - 1
 *   float:  f16_rn(f32(v))                                    no clamp
 * Errors: null pointers, negative sizes, C outside 1..8, a dtype code outside 0..2: MIXDQ_ERR_INVALID_ARG; out not
 * 16-byte aligned or img not aligned to its element: MIXDQ_ERR_ALIGNMENT.  B * H * W == 0 writes nothing (and looks at
 * no pointer: an empty tensor has no storage).
 *
 * mixdq_vae_latent_sample: the posterior sample.  moments: FP16 [B, h, w, 2L] (channels 0..L-1 the mean, L..2L-1 the
 * log-variance), noise: FP32 [B, h, w, L] or null, z: FP32 [B, h, w, L]; `pixels` = B * h * w.
 *   z = (f32(mean) + exp(0.5 * clamp(f32(logvar), -30, 20)) * noise) * scaling_factor
 *   noise == null:  z = f32(mean) * scaling_factor                  (the mode of the posterior)
 * every operation one FP32 rounding, never contracted (include/mixdq_math.h: mixdq_vae_latent[_mode]).
 * L % 4 == 0 and 16-byte aligned pointers: MIXDQ_ERR_ALIGNMENT otherwise; null moments / z, pixels < 0, L < 1:
 * MIXDQ_ERR_INVALID_ARG.  pixels == 0 writes nothing.
 *
 * mixdq_image_to_nhwc8_f16_masked: the same ingest with the masked pixels blanked, for the 9-channel inpainting
 * checkpoints' "masked image".  mask: [B, H, W] at image resolution, dtype code and element strides mb, mh, mw as
 * mixdq_composite_u8 takes them, SET by the rule below (uint8 u >= 128, floats v >= 0.5, NaN not set):
 *   out[b, y, x, c] = set(mask[b, y, x]) ? +0.0 : ingest(img[b, c, y, x])      c < C;   channels C..7 zero
 * with `ingest` the arithmetic above, unchanged; one 16-byte store per pixel.  It is diffusers'
 * init_image * (mask < 0.5) in model space: a blanked pixel is mid-grey (0.0), not black (-1.0).  It differs from that
 * product only where the product is not +0.0 under a set mask: diffusers leaves -0.0 for a negative source and NaN
 * for a non-finite one, this kernel stores +0.0.  An all-clear mask gives mixdq_image_to_nhwc8_f16's bits.
 * Errors: as mixdq_image_to_nhwc8_f16, and a mask dtype code outside 0..2 or a null mask: MIXDQ_ERR_INVALID_ARG; mask
 * not aligned to its element: MIXDQ_ERR_ALIGNMENT.  B * H * W == 0 writes nothing (and looks at no pointer).
 *
 * mixdq_inpaint_cond_f16: the conditioning channels of a 9-channel inpainting UNet in the padded 8-channel form
 * SDXLUNet.cond_term takes.  mask_lat: FP32 [B, h, w] dense (mixdq_mask_to_latent's output, or a soft mask: the values
 * pass through), zl: FP32 [B, h, w, L] dense (mixdq_vae_latent_sample's output for the blanked image), out: FP16
 * [B, h, w, 8]; `pixels` = B * h * w.
 *   out[p, 0] = f16_rn(mask_lat[p]);   out[p, 1 + l] = f16_rn(zl[p, l]), l < L;   out[p, L + 1 .. 7] = +0.0
 * One 16-byte store per latent pixel.  1 <= L <= 7.
 * Errors: pixels < 0, L outside 1..7, null pointers: MIXDQ_ERR_INVALID_ARG; out not 16-byte aligned, mask_lat or zl
 * not 4-byte aligned: MIXDQ_ERR_ALIGNMENT.  pixels == 0 writes nothing (and looks at no pointer).
 *
 * mixdq_ip2p_cond_f16: the conditioning channels of an 8-channel InstructPix2Pix UNet in the same padded form, one row
 * block per UNet row block (mixdq_sampler_step3's order: text + image, image only, neither).  moments: FP16
 * [B, h, w, 2L] dense (the VAE encoder's output in memory: L means, then L log-variances, which are not read), out:
 * FP16 [rows * B, h, w, 8], rows 1 or 3; pixels_per_image = h * w.  With p a pixel of image b:
 *   out[r * B + b, p, l] = f16_rn(f32(mean[b, p, l]) * scale)      l < L, r < min(rows, 2)
 *   every other channel, and the whole third block                 +0.0
 * one FP32 rounding (include/mixdq_math.h: mixdq_vae_latent_mode), then the FP16 one: scale 1.0f returns the mean's own
 * bits -- latent_dist.mode() unscaled, what both diffusers pipelines feed; CosXL-Edit multiplies by scaling_factor.  One
 * 16-byte store per output pixel.  1 <= L <= 8.
 * Errors: B < 0, pixels_per_image < 0, L outside 1..8, rows not 1 or 3, null pointers: MIXDQ_ERR_INVALID_ARG; out not
 * 16-byte, moments not 2-byte aligned: MIXDQ_ERR_ALIGNMENT.  B * pixels_per_image == 0 writes nothing (and looks at no
 * pointer). */
#define MIXDQ_IMAGE_U8 0
#define MIXDQ_IMAGE_F16 1
#define MIXDQ_IMAGE_F32 2
int mixdq_image_to_nhwc8_f16(const void* img, int dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                             void* out_f16, int B, int C, int H, int W, mixdq_stream_t stream);
int mixdq_vae_latent_sample(const void* moments_f16, const float* noise_or_null, float* z, int64_t pixels, int L,
                            float scaling_factor, mixdq_stream_t stream);
int mixdq_image_to_nhwc8_f16_masked(const void* img, int dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                                    const void* mask, int mask_dtype, int64_t mb, int64_t mh, int64_t mw,
                                    void* out_f16, int B, int C, int H, int W, mixdq_stream_t stream);
int mixdq_inpaint_cond_f16(const float* mask_lat, const float* zl, void* out_f16, int64_t pixels, int L,
                           mixdq_stream_t stream);
int mixdq_ip2p_cond_f16(const void* moments_f16, void* out_f16, int B, int64_t pixels_per_image, int L, int rows,
                        float scale, mixdq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Inpainting around the VAE (csrc/vae.hip).  No reference counterpart.  A mask value is SET (repaint) by
 * diffusers' rule: uint8 u >= 128 (u / 255 >= 0.5), FP16 / FP32 v >= 0.5; NaN is not set.
 *
 * mixdq_mask_to_latent: an image-resolution mask as the latent-resolution mask the masked sampler step reads.
 * mask: [B, H, W] of uint8 / FP16 / FP32 (the MIXDQ_IMAGE_* codes), element (b, y, x) at mask + (b * sb + y * sh +
 * x * sw) ELEMENTS; out: FP32 [B, H/8, W/8] dense, every value exactly 0.0 or 1.0.
 *   MIXDQ_MASK_NEAREST  out[b, i, j] = set(mask[b, 8i, 8j])      what F.interpolate(mask, size=(H/8, W/8)) in its
 *                                                                default nearest mode picks: diffusers' pipeline
 *   MIXDQ_MASK_ANY      out[b, i, j] = any pixel of rows 8i..8i+7, columns 8j..8j+7 set: a latent whose block
 *                       touches the mask is repainted.  Rows are read with 8- / 16-byte loads where sw == 1 and the
 *                       pointer, sh and sb keep every row start aligned, element by element otherwise.
 * Errors: negative sizes, H % 8 or W % 8 nonzero, a dtype code outside 0..2, an unknown mode, null pointers:
 * MIXDQ_ERR_INVALID_ARG; mask not aligned to its element or out to 4 bytes: MIXDQ_ERR_ALIGNMENT.  B * H * W == 0
 * writes nothing (and looks at no pointer).
 *
 * mixdq_composite_u8: the decoded image pasted into the original under the mask, as pixels:
 *   out[b, y, x, c] = set(mask[b, y, x]) ? mixdq_to_uint8(f32(decoded[b, c, y, x])) : original[b, c, y, x]     c < 3
 * decoded: FP16, element (b, c, y, x) at decoded + (b * db + c * dc + y * dh + x * dw) elements (VAEDecoder.decode
 * returns three channels of a four-channel channels-last tensor: strides say so); original: uint8, strides ob, oc,
 * oh, ow likewise; mask: at image resolution, dtype code and strides mb, mh, mw as above; out: uint8 [B, H, W, 3]
 * dense.  mixdq_to_uint8 (include/mixdq_math.h) is ((v / 2 + 0.5).clamp(0, 1) * 255).round(), half to even, NaN 0.
 * Pixels outside the mask are the original's bytes.
 * Errors: negative sizes, a mask dtype code outside 0..2, null pointers: MIXDQ_ERR_INVALID_ARG; decoded or mask not
 * aligned to its element: MIXDQ_ERR_ALIGNMENT.  B * H * W == 0 writes nothing (and looks at no pointer). */
#define MIXDQ_MASK_NEAREST 0
#define MIXDQ_MASK_ANY 1
int mixdq_mask_to_latent(const void* mask, int dtype, int64_t sb, int64_t sh, int64_t sw, float* out, int B, int H,
                         int W, int mode, mixdq_stream_t stream);
int mixdq_composite_u8(const void* decoded_f16, int64_t db, int64_t dc, int64_t dh, int64_t dw,
                       const uint8_t* original, int64_t ob, int64_t oc, int64_t oh, int64_t ow, const void* mask,
                       int mask_dtype, int64_t mb, int64_t mh, int64_t mw, uint8_t* out, int B, int H, int W,
                       mixdq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Separable resampling (csrc/image.hip): resize, mask blur and the crop workflow's paste are one filter kernel over
 * host-made tables.  No reference counterpart.  Arithmetic: include/mixdq_math.h (mixdq_resample_tap, mixdq_round_u8,
 * mixdq_blend_u8, mixdq_to_uint8): the horizontal chain of every source row first, then the vertical chain, FP32 fused
 * multiply-adds in tap order, zero weights skipped.
 *
 * Tables (device memory): xs int32 [Bt, Wd], wx float [Bt, Wd, Tx], ys int32 [Bt, Hd], wy float [Bt, Hd, Ty]; Bt is 1
 * (one table for the batch) or B (one per image); 1 <= Tx, Ty <= 256.  Tap i of output column x reads source column
 * min(max(xs[x] + i, 0), Ws - 1) with weight wx[x][i], rows likewise: a bad table gives wrong pixels, never an access
 * out of bounds.
 *
 * mixdq_resample: src [B, C, Hs, Ws] of uint8 / FP16 / FP32 (MIXDQ_IMAGE_*), element (b, c, y, x) at src + (b * sb +
 * c * sc + y * sh + x * sw) ELEMENTS, C in 1..4; dst dense [B, Hd, Wd, C].
 *   src_mode  MIXDQ_RESAMPLE_SRC_VALUE  an element enters as (float)u (uint8) or as its value (FP16 / FP32)
 *             MIXDQ_RESAMPLE_SRC_MASK   as 255.0f where it is set (u >= 128, v >= 0.5; NaN is not), 0.0f elsewhere
 *   dst_kind  MIXDQ_RESAMPLE_DST_U8       uint8, mixdq_round_u8(acc)
 *             MIXDQ_RESAMPLE_DST_U8_UNIT  uint8, mixdq_to_uint8(acc): a source in [-1, 1] (a decoded image) as pixels
 *             MIXDQ_RESAMPLE_DST_F32      float, the accumulator itself
 * Errors: negative sizes, C outside 1..4, Tx / Ty outside 1..256, Bt neither 1 nor B, an unknown dtype, src_mode or
 * dst_kind, an output without a source (Hs * Ws == 0), null pointers: MIXDQ_ERR_INVALID_ARG; src not aligned to its
 * element, a table or an F32 dst not to 4 bytes: MIXDQ_ERR_ALIGNMENT.  B * Hd * Wd == 0 writes nothing (and looks at
 * no pointer).
 *
 * mixdq_resample_paste_u8: the way back of the crop workflow in one launch.  decoded: FP16 [B, 3, Hm, Wm] at element
 * strides db, dc, dh, dw; out: uint8 [B, H, W, 3] dense, holding the original, updated IN PLACE; win: int32 [B, 4] =
 * (x0, y0, x1, y1), image b's half-open window in out; tables as above with Wd = Wt, Hd = Ht (the largest window of
 * the batch) indexed by the window-relative coordinate, the source extents being Wm and Hm.  For every pixel (x, y)
 * of image b with x0 <= x < min(x1, x0 + Wt, W), rows likewise, and every c < 3:
 *   out[b, y, x, c] = mixdq_blend_u8(m, mixdq_to_uint8(acc), out[b, y, x, c])
 * mask [B, H, W] at element strides mb, mh, mw:
 *   MIXDQ_PASTE_MASK_BINARY  any MIXDQ_IMAGE_* dtype, m = set ? 255 : 0
 *   MIXDQ_PASTE_MASK_SOFT    uint8 only, m = the byte
 * Nothing outside a window (or outside the image, whatever win says) is written; inside, a byte with m = 0 is written
 * back unchanged; each byte is read and written by the same lane.
 * Errors: as above, and SOFT with a mask that is not uint8: MIXDQ_ERR_INVALID_ARG; decoded or mask not aligned to its
 * element, win or a table not to 4 bytes: MIXDQ_ERR_ALIGNMENT.  B * Ht * Wt == 0 or B * H * W == 0 writes nothing.
 *
 * mixdq_mask_bbox: mask [B, H, W] (MIXDQ_IMAGE_*, strides sb, sh, sw) -> out int32 [B, 4] = (x0, y0, x1, y1), the
 * half-open bounding box of the set pixels, (0, 0, 0, 0) where none is set.  One workgroup per image; not a hot path
 * (it runs once, in front of a host read-back).  Errors: negative sizes, an unknown dtype, null pointers:
 * MIXDQ_ERR_INVALID_ARG; mask not aligned to its element, out not to 4 bytes: MIXDQ_ERR_ALIGNMENT.  B * H * W == 0
 * writes nothing.
 *
 * mixdq_mask_dilate_u8: a mask grown by `radius` pixels (front ends' "grow mask by").  mask [B, H, W] (MIXDQ_IMAGE_*,
 * element strides sb, sh, sw) -> out uint8 [B, H, W] dense:
 *   out[b, y, x] = 255 where any pixel of rows max(y - r, 0) .. min(y + r, H - 1), columns max(x - r, 0) ..
 *                  min(x + r, W - 1) of image b is set (u >= 128, v >= 0.5; NaN is not), 0 elsewhere
 * -- the square window of PIL's ImageFilter.MaxFilter(2r + 1) on the binarised mask, exact; a window never reaches
 * into another image of the batch.  0 <= radius <= 255; radius 0 is the binarisation, a radius beyond the image is
 * legal.  Two launches: rows (mask -> scratch), then columns (scratch -> out); scratch: uint8 [B, H, W] of the
 * caller's, overwritten, distinct from out.  Not a hot path (once per call, in front of the whole pipeline).
 * Errors: negative sizes, an unknown dtype, radius outside 0..255, null pointers: MIXDQ_ERR_INVALID_ARG; mask not
 * aligned to its element: MIXDQ_ERR_ALIGNMENT.  B * H * W == 0 writes nothing (and looks at no pointer). */
#define MIXDQ_RESAMPLE_SRC_VALUE 0
#define MIXDQ_RESAMPLE_SRC_MASK 1
#define MIXDQ_RESAMPLE_DST_U8 0
#define MIXDQ_RESAMPLE_DST_U8_UNIT 1
#define MIXDQ_RESAMPLE_DST_F32 2
#define MIXDQ_PASTE_MASK_BINARY 0
#define MIXDQ_PASTE_MASK_SOFT 1
#define MIXDQ_RESAMPLE_MAX_TAPS 256
int mixdq_resample(const void* src, int dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int src_mode, void* dst,
                   int dst_kind, const int32_t* xs, const float* wx, int Tx, const int32_t* ys, const float* wy, int Ty,
                   int Bt, int B, int C, int Hs, int Ws, int Hd, int Wd, mixdq_stream_t stream);
int mixdq_resample_paste_u8(const void* decoded_f16, int64_t db, int64_t dc, int64_t dh, int64_t dw, int Hm, int Wm,
                            uint8_t* out, const void* mask, int mask_dtype, int64_t mb, int64_t mh, int64_t mw,
                            int mask_mode, const int32_t* win, const int32_t* xs, const float* wx, int Tx,
                            const int32_t* ys, const float* wy, int Ty, int Bt, int Ht, int Wt, int B, int H, int W,
                            mixdq_stream_t stream);
int mixdq_mask_bbox(const void* mask, int dtype, int64_t sb, int64_t sh, int64_t sw, int32_t* out, int B, int H, int W,
                    mixdq_stream_t stream);
int mixdq_mask_dilate_u8(const void* mask, int dtype, int64_t sb, int64_t sh, int64_t sw, uint8_t* scratch,
                         uint8_t* out, int B, int H, int W, int radius, mixdq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Sampler step: classifier-free guidance + scheduler update + the UNet's next input, and the step state kept on
 * the device, so that a sampling loop is N replays of one captured graph with nothing from the host in between.
 * No reference counterpart: the reference reaches the loop only through diffusers' pipeline call in its run()
 * harness (quantize_sdxl.py:331-484); schedulers and guidance are diffusers' eager PyTorch ops there.
 * Euler, Euler-ancestral, DDIM and LCM updates of an epsilon-predicting model are one affine map; with
 * (a, b, c, s_next) = coef[*step] (coef: FP32 [n_steps][4], 16-byte aligned), per element i < n:
 *   e      = f32(eps[i])                                                   rows_per_image == 1
 *   e      = f32(eps[i]) + g * (f32(eps[row_stride + i]) - f32(eps[i]))    rows_per_image == 2
 *   x[i]   = (a * x[i] + b * e) + c * noise[*step * noise_stride + i]      (noise == null: a * x[i] + b * e)
 *   in[i]  = in[row_stride + i] (rows_per_image == 2) = f16_rn(x[i] * s_next)
 * every operation FP32 round-to-nearest, never contracted (include/mixdq_math.h: mixdq_sampler_*).  x: the FP32
 * latent state, updated in place; eps: the UNet's FP16 output -- unconditional rows first, the conditional rows
 * row_stride elements behind them; in: the UNet's FP16 input buffer, same layout.  The kernel is elementwise over
 * storage: x, noise, eps and in share ONE dense stride pattern (the Python layer: channels-last).  n need not be
 * a multiple of 8.  Then, in a one-thread launch behind the step on the same stream (in-order execution is what
 * keeps every workgroup of the step from seeing the moved index):
 *   *timestep = t_table[*step + 1];  *step += 1             (t_table: FP32 [n_steps + 1])
 * A call with *step outside [0, n_steps) reads and writes nothing.
 * Errors: null pointers, n < 0, n_steps < 1, rows_per_image not 1 or 2, row_stride < n (rows_per_image == 2),
 * noise_stride < n (with noise): MIXDQ_ERR_INVALID_ARG; x / eps / in / noise / coef not 16-byte aligned,
 * row_stride % 8 != 0 (rows_per_image == 2), noise_stride % 4 != 0 (with noise): MIXDQ_ERR_ALIGNMENT. */
int mixdq_sampler_step(float* x, const void* eps_f16, void* in_f16, const float* noise_or_null,
                       int64_t noise_stride, const float* coef, const float* t_table, int n_steps,
                       int* step, float* timestep, float guidance, int64_t n, int rows_per_image,
                       int64_t row_stride, mixdq_stream_t stream);

/* The same step for inpainting with a 4-channel UNet (diffusers' StableDiffusion[XL]InpaintPipeline when
 * num_channels_unet == 4): after the update above, the region the mask keeps is overwritten with the image latents
 * noised to the NEXT step's level.  With x' the value mixdq_sampler_step would store, (p, q) = blend[*step] (blend:
 * FP32 [n_steps][2], 8-byte aligned: the scheduler's add_noise scalars at timestep *step + 1, the last row (1, 0))
 * and m = mask[i / channels]:
 *   k      = (p * z[i]) + (q * noise0[i])
 *   x[i]   = ((1 - m) * k) + (m * x')                     m = 1 repaints, m = 0 keeps, values between blend
 *   in[i]  = in[row_stride + i] (rows_per_image == 2) = f16_rn(x[i] * s_next)
 * every operation FP32 round-to-nearest, never contracted (include/mixdq_math.h: mixdq_sampler_blend).  z: the image
 * latents and noise0: the run's initial noise (diffusers re-uses it at every step), FP32, n elements each in x's
 * stride pattern; mask: FP32, one value per latent pixel, [B, h, w] dense, n / channels entries -- element i of
 * the channels-last storage belongs to entry i / channels.  Any channels >= 1 with n % channels == 0; n need not be
 * a multiple of 8.  The advance launch behind it and the behaviour past the table are mixdq_sampler_step's.
 * Errors: mixdq_sampler_step's, then null z / noise0 / mask / blend, channels < 1, n % channels != 0:
 * MIXDQ_ERR_INVALID_ARG; z / noise0 not 16-byte, mask not 4-byte, blend not 8-byte aligned: MIXDQ_ERR_ALIGNMENT.
 * A refused call launches nothing. */
int mixdq_sampler_step_masked(float* x, const void* eps_f16, void* in_f16, const float* noise_or_null,
                              int64_t noise_stride, const float* coef, const float* t_table, int n_steps,
                              int* step, float* timestep, float guidance, int64_t n, int rows_per_image,
                              int64_t row_stride, const float* z, const float* noise0, const float* mask,
                              int channels, const float* blend, mixdq_stream_t stream);

/* The step of a two-step multistep solver, DPM-Solver++ 2M (diffusers' DPMSolverMultistepScheduler, epsilon
 * prediction, solver_order 2, midpoint): the one update rule here that is not an affine map of (x, eps, noise), because
 * a second-order step also needs the previous step's data prediction.  hist: FP32, n elements in x's stride pattern,
 * 16-byte aligned, a buffer of its own (it may not overlap x) -- that previous prediction; coef8: FP32 [n_steps][8],
 * 16-byte aligned, row i = (u, v, A, B1, B2, D2, s_next, 0); first: a device int32 holding the index of the first step
 * of this run (0, or an image-to-image run's start).  With e the guided epsilon as above, per element i < n:
 *   x0      = (u * x[i]) + (v * e)                                          the data prediction
 *   second  = *step > *first && D2 != 0                                     the same for every element of the launch
 *   x[i]    = second ? ((A * x[i]) + (B2 * x0)) + (D2 * hist[i]) : (A * x[i]) + (B1 * x0)
 *   hist[i] = x0                                                            on EVERY step, first-order ones included
 *   in[i]   = in[row_stride + i] (rows_per_image == 2) = f16_rn(x[i] * s_next)
 * every operation FP32 round-to-nearest, never contracted (include/mixdq_math.h: mixdq_sampler_x0,
 * mixdq_sampler_update_2m, mixdq_sampler_update).  On a first-order step hist is not read: before the first step of a
 * run it may hold anything, NaN included, and nothing has to clear it between runs.  These kinds add no noise: there
 * is no noise operand.  The advance launch behind the step and the behaviour past the table (nothing read or written,
 * hist included) are mixdq_sampler_step's.
 * Errors: mixdq_sampler_step's (coef8 in coef's place), then null hist / first, hist overlapping x:
 * MIXDQ_ERR_INVALID_ARG; hist / coef8 not 16-byte, first not 4-byte aligned: MIXDQ_ERR_ALIGNMENT. */
int mixdq_sampler_step_2m(float* x, const void* eps_f16, void* in_f16, float* hist, const float* coef8,
                          const float* t_table, int n_steps, int* step, const int* first, float* timestep,
                          float guidance, int64_t n, int rows_per_image, int64_t row_stride, mixdq_stream_t stream);

/* mixdq_sampler_step_2m for inpainting: with x' the value it would store, x[i] = mixdq_sampler_step_masked's blend of
 * x' with (p, q) = blend[*step] and m = mask[i / channels], and in[i] is taken from that.  hist[i] is x0 as above,
 * NOT blended: the solver's history is the model's prediction (diffusers' pipeline overwrites the latents after
 * scheduler.step and leaves the scheduler's model_outputs alone).  z, noise0, mask, channels, blend and their errors
 * as in mixdq_sampler_step_masked, after mixdq_sampler_step_2m's. */
int mixdq_sampler_step_2m_masked(float* x, const void* eps_f16, void* in_f16, float* hist, const float* coef8,
                                 const float* t_table, int n_steps, int* step, const int* first, float* timestep,
                                 float guidance, int64_t n, int rows_per_image, int64_t row_stride, const float* z,
                                 const float* noise0, const float* mask, int channels, const float* blend,
                                 mixdq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Gaussian noise made on the device: Philox4x32-10, a counter-based generator, and Box-Muller on 24-bit uniforms
 * (include/mixdq_math.h: mixdq_philox4x32_10, mixdq_rng_*; integers and FP32 with every rounding explicit, so the
 * values can be restated bit for bit on a host).  No reference counterpart (the reference takes torch's generator
 * through diffusers).  Image b of a batch has a 64-bit seed seeds[b] (device memory, 8-byte aligned, read as unsigned);
 * element e of that image, counted in storage (NHWC) order, is output lane e & 3 of the call with
 *   key (lo32(seed), hi32(seed)),  counter (lo32(e >> 2), hi32(e >> 2), step, stream)
 * stream: what the noise is for (below); step: the absolute index of the sampler step that consumes it (stream 1), 0
 * for the others.  An image's noise depends on its seed and size only -- not on its batch position, the batch size,
 * the launch geometry or where a run starts in the schedule.  |z| <= sqrt(48 ln 2) ~ 5.77. */
#define MIXDQ_RNG_STREAM_START 0   /* start noise; the img2img / inpainting noise */
#define MIXDQ_RNG_STREAM_STEP 1    /* what a stochastic sampler step adds */
#define MIXDQ_RNG_STREAM_VAE 2     /* the VAE posterior's noise */
#define MIXDQ_RNG_STREAM_COND 3    /* the posterior's noise of the blanked image a 9-channel inpainting UNet reads */

/* out[b * n_image + e] for b < B, e < n_image, dense.  Any n_image >= 1; out 16-byte aligned when n_image % 4 == 0
 * (16-byte stores), 4-byte otherwise.  The seeds are read by the kernel: a captured graph serves every seed.
 * Errors: null out / seeds, B < 0, n_image < 1: MIXDQ_ERR_INVALID_ARG; out or seeds misaligned: MIXDQ_ERR_ALIGNMENT.
 * B == 0 writes nothing. */
int mixdq_randn_f32(float* out, int B, int64_t n_image, const uint64_t* seeds_device, uint32_t stream, uint32_t step,
                    mixdq_stream_t hip_stream);

/* Introspection (tests): the map from raw words to normals alone -- z[4 q .. 4 q + 3] = mixdq_rng_normals4(r[4 q ..
 * 4 q + 3]) for q < n_quads; r and z 16-byte aligned device memory. */
int mixdq_rng_normals_from_bits(const uint32_t* r, float* z, int64_t n_quads, mixdq_stream_t stream);

/* mixdq_sampler_step / mixdq_sampler_step_masked with the noise of stochastic steps computed in registers instead of
 * read from a buffer: n[i] = the normal of (seeds[i / n_image], element i % n_image, step *step, stream
 * MIXDQ_RNG_STREAM_STEP), the values mixdq_randn_f32(.., MIXDQ_RNG_STREAM_STEP, *step) writes -- then exactly the
 * sibling's arithmetic with that n.  seeds (n / n_image entries) and n_image take the place of noise and
 * noise_stride; everything else is the sibling's, in its order.  n_image % 8 == 0: an 8-element pass lies inside one
 * image and takes two Philox calls; other n_image: one call per element.
 * Errors: the sibling's, then null seeds, n_image < 1, n % n_image != 0: MIXDQ_ERR_INVALID_ARG; seeds not 8-byte
 * aligned: MIXDQ_ERR_ALIGNMENT. */
int mixdq_sampler_step_rng(float* x, const void* eps_f16, void* in_f16, const uint64_t* seeds, int64_t n_image,
                           const float* coef, const float* t_table, int n_steps, int* step, float* timestep,
                           float guidance, int64_t n, int rows_per_image, int64_t row_stride, mixdq_stream_t stream);
int mixdq_sampler_step_masked_rng(float* x, const void* eps_f16, void* in_f16, const uint64_t* seeds, int64_t n_image,
                                  const float* coef, const float* t_table, int n_steps, int* step, float* timestep,
                                  float guidance, int64_t n, int rows_per_image, int64_t row_stride, const float* z,
                                  const float* noise0, const float* mask, int channels, const float* blend,
                                  mixdq_stream_t stream);

/* The step with THREE UNet rows per image and two guidance scales: InstructPix2Pix (diffusers'
 * StableDiffusion[XL]InstructPix2PixPipeline).  eps and in hold three row blocks row_stride elements apart, in those
 * pipelines' order -- NOT the two-row convention, where the unconditional block comes first:
 *   block 0: text + image (e_t)      block 1: image only (e_i)      block 2: neither (e_u)
 *   e     = (e_u + g * (e_t - e_i)) + gi * (e_i - e_u)              g = guidance, gi = image_guidance
 *   in[i] = in[row_stride + i] = in[2 * row_stride + i] = f16_rn(x[i] * s_next)
 * six roundings, FP32 round-to-nearest, never contracted (include/mixdq_math.h: mixdq_sampler_guided_eps3); everything
 * behind the guided epsilon -- update, history, blend, scaled input, the advance launch, the behaviour past the table --
 * is the sibling's of the same mode.  This ONE entry point takes the whole operand set flat; the operands of a mode
 * are null when the mode is off:
 *   table, table_width       coef and 4, or coef8 and 8 (DPM-Solver++ 2M: then hist and first, and no noise)
 *   noise_or_null / noise_stride, seeds_or_null / n_image       at most one of the two, width 4 only
 *   hist_or_null / first_or_null                                both with width 8, neither with width 4
 *   z / noise0 / mask / blend (+ channels)                      all four (the masked step) or none
 * Errors, before any launch: table_width not 4 or 8, width 8 with noise or seeds, noise and seeds together, width 8
 * without hist / first (or width 4 with one): MIXDQ_ERR_INVALID_ARG; then the siblings' checks in their order, with
 * row_stride >= n and row_stride % 8 == 0 as for two rows.  The six entry points above keep refusing
 * rows_per_image == 3. */
int mixdq_sampler_step3(float* x, const void* eps_f16, void* in_f16, const float* table, int table_width,
                        const float* t_table, int n_steps, int* step, float* timestep, float guidance,
                        float image_guidance, int64_t n, int64_t row_stride, const float* noise_or_null,
                        int64_t noise_stride, const uint64_t* seeds_or_null, int64_t n_image, float* hist_or_null,
                        const int* first_or_null, const float* z, const float* noise0, const float* mask, int channels,
                        const float* blend, mixdq_stream_t stream);

/* Guidance rescale (csrc/sampler_rescale.hip; diffusers' guidance_rescale, Lin et al. 2023): the step of the entry
 * points above at two or three rows per image, with the guided model output e of every image multiplied by
 *   r = 1 + rescale * (sqrt(M2_t / M2_e) - 1),      M2_v = sum over the image's n_image elements of (v - mean_v)^2
 * before the update -- t the text-conditioned output (two rows: row block 1; three rows: block 0), so that sqrt(M2_t /
 * M2_e) is std(t) / std(e) of torch's unbiased std.  r = 1 where M2_e == 0, M2_t == 0 or n_image == 1 (diffusers
 * returns NaN there).  How M2 is summed -- chunks of 2048 elements, a fixed order inside a chunk, Chan's update across
 * them -- is part of the specification: include/mixdq_math.h, mixdq_rescale_*.  With rescale == 0 (r == 1 exactly) the
 * results are the sibling entry point's bit for bit.
 * ONE entry point, the whole operand set flat as mixdq_sampler_step3 takes it (the operands of a mode null when the
 * mode is off), and beside it: rows_per_image 2 (image_guidance is not read) or 3; rescale, phi in [0, 1]; n_image, the
 * elements of one image (n = images * n_image; also what seeds_or_null counts by); workspace, FP32 device memory of
 * mixdq_sampler_rescale_workspace_floats(n, n_image) floats, 16-byte aligned, the caller's: nothing is allocated here,
 * its contents need not survive between calls.  Launches, in stream order on grids of exactly (ceil(n_image / 2048),
 * images) workgroups: the chunk statistics, the step (which combines them per image), the advance; n == 0: the advance
 * alone.
 * Errors, before any launch: rows_per_image not 2 or 3, then mixdq_sampler_step3's own and the siblings' checks in
 * their order; then rescale outside [0, 1] or NaN, n_image < 1, n % n_image != 0, a null workspace, more than 65535
 * images (the grid's y extent): MIXDQ_ERR_INVALID_ARG; workspace not 16-byte aligned: MIXDQ_ERR_ALIGNMENT.
 * mixdq_sampler_rescale_workspace_floats: 0 for n < 0, n_image < 1 or n % n_image != 0. */
size_t mixdq_sampler_rescale_workspace_floats(int64_t n, int64_t n_image);
int mixdq_sampler_step_rescaled(float* x, const void* eps_f16, void* in_f16, const float* table, int table_width,
                                const float* t_table, int n_steps, int* step, float* timestep, float guidance,
                                float image_guidance, float rescale, int rows_per_image, int64_t n, int64_t n_image,
                                int64_t row_stride, float* workspace, const float* noise_or_null, int64_t noise_stride,
                                const uint64_t* seeds_or_null, float* hist_or_null, const int* first_or_null,
                                const float* z, const float* noise0, const float* mask, int channels,
                                const float* blend, mixdq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * ControlNet glue (csrc/control.hip).  No reference counterpart: the reference's UNet wrapper passes diffusers'
 * down_block_additional_residuals / mid_block_additional_residual through.
 *
 * mixdq_control_add_f16: every skip tensor of a UNet (the mid-block output included) plus the scaled residuals of K
 * ControlNets, in ONE launch.  S segments (1..16), K nets (1..4); segment i has n[i] FP16 elements, skip[i], dst[i] and
 * the residuals residuals[k * S + i] of net k.  skip, dst, residuals and n are HOST arrays, read during the call: the
 * descriptors travel in the kernel arguments, so a captured graph holds them and nothing is copied to the device.
 * scales: FP32 [K, n_steps] on the device; step: the int32 on the device that mixdq_sampler_step* advances, read by the
 * kernel.  With c_k = scales[k * n_steps + *step], element e of segment i (include/mixdq_math.h, mixdq_control_*):
 *   t_k = f16_rn(f32(r_k[e]) * c_k), nets in the order k = 0 .. K-1, a net with c_k == 0 skipped and its residual not read
 *   acc = t_first;  acc = f16_rn(f32(acc) + f32(t_k)) for each later net
 *   dst[e] = f16_rn(f32(skip[e]) + f32(acc));   every net skipped: dst[e] = skip[e]'s own bits
 * -- diffusers' ControlNetModel / MultiControlNetModel / UNet arithmetic on FP16 tensors, except that a scale of exactly
 * 0 skips the net where diffusers computes r * 0 (different only for a non-finite r and in the sign of a zero).  *step
 * outside [0, n_steps) reads every scale as 0: dst = skip.  dst is always written; dst[i] may be skip[i] itself.
 * Grid: exactly sum(ceil(n[i] / mixdq_control_chunk())) workgroups of 256 lanes; 16-byte accesses.
 * Errors, before any launch: S or K out of range, n_steps < 1, a null array, scales or step, n[i] < 0, a null pointer of
 * a segment with n[i] > 0: MIXDQ_ERR_INVALID_ARG; n[i] % 8 != 0, a segment pointer not 16-byte or scales / step not
 * 4-byte aligned: MIXDQ_ERR_ALIGNMENT.  A segment with n[i] == 0 contributes no workgroup (its pointers are not looked
 * at); all empty: nothing is launched.
 *
 * mixdq_silu_f16: out[e] = f16_rn(mixdq_siluf(f32(x[e]))), n elements; out may be x.  n % 8 == 0 and 16-byte aligned
 * pointers (MIXDQ_ERR_ALIGNMENT otherwise); n < 0, null pointers: MIXDQ_ERR_INVALID_ARG; n == 0 writes nothing.  Grid:
 * exactly ceil(n / 2048) workgroups of 256 lanes.
 *
 * mixdq_hint_to_nhwc8_f16: a ControlNet's image ingest -- mixdq_image_to_nhwc8_f16's interface, layouts and errors,
 * with the [0, 1] rule:
 *   uint8:  f16_rn(f32(u) / 255.0f)        the division correctly rounded: image.float() / 255, then .half()
 *   float:  f16_rn(f32(v))                 no clamp
 * Grid: exactly ceil(B * H * W / 256) workgroups of 256 lanes, one pixel and one 16-byte store per lane. */
#define MIXDQ_CONTROL_MAX_SEGMENTS 16
#define MIXDQ_CONTROL_MAX_NETS 4
int mixdq_control_chunk(void);
int mixdq_control_add_f16(const void* const* skip, void* const* dst, const void* const* residuals, const int64_t* n,
                          int S, int K, const float* scales, int n_steps, const int* step, mixdq_stream_t stream);
int mixdq_silu_f16(const void* x_f16, void* out_f16, int64_t n, mixdq_stream_t stream);
int mixdq_hint_to_nhwc8_f16(const void* img, int dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw, void* out_f16,
                            int B, int C, int H, int W, mixdq_stream_t stream);

/* Which kernel instantiation mixdq_qlinear_w8a8 / mixdq_qconv2d_w8a8 will launch for a problem of
 * M rows x N output channels (k_align = K for Linear, C for Conv2d; k_total = K or R*S*C): the block tile BM x BN x BK
 * and LDS stage count of `igemm_kernel<BM,BN,BK,STAGES,CONV>`, or zeros for the small-alignment
 * generic kernel.  Host-only
 * query, used by bench.py to attribute measured time to kernel names.  No reference counterpart. */
int mixdq_igemm_select(int64_t M, int N, int k_align, int k_total, int* bm, int* bn, int* bk,
                       int* stages);
/* The configuration id behind mixdq_igemm_select (the ids of MIXDQ_IGEMM_CONFIGS in csrc/igemm.hip,
 * which bits 8..15 of `flags` can force; 0 = the small-alignment generic kernel, -1 = invalid):
 * two ids may share a tile shape and differ in the number of waves working on it. */
int mixdq_igemm_select_id(int64_t M, int N, int k_align, int k_total);
/* The same for a packed-W4 weight operand (MIXDQ_FLAG_W4); -1 = invalid (k_align % 32 != 0). */
int mixdq_igemm_select_id_w4(int64_t M, int N, int k_align, int k_total);
/* The same for a packed-W2 weight operand (MIXDQ_FLAG_W2); -1 = invalid (K % 64 != 0).  Never one of the
 * ids W2 cannot take (27, 42, 43, 44, 45, 56). */
int mixdq_igemm_select_id_w2(int64_t M, int N, int k_align, int k_total);
/* The same for the GEMM + GEGLU + quantize launch (mixdq_qlinear_w8a8_geglu), whose tiles hold whole
 * 32-column value | gate groups (BN % 32 == 0); from 1.5 workgroups of 256x256 per CU on it runs on the
 * four-phase 256x256 tile (id 70) like a plain Linear. */
int mixdq_igemm_select_id_geglu(int64_t M, int N, int k_total, int w4);
/* ... and for the GEMM + GEGLU launch on packed-W2 weights; -1 = invalid (N % 32 or K % 64 != 0). */
int mixdq_igemm_select_id_geglu_w2(int64_t M, int N, int k_total);

/* Tile configurations this library was compiled with.  family: 0 INT8 GEMM/conv (all ids), 1 FP16,
   2 grouped, 3 quantize-in-prologue (f16in), 5 LDS-halo conv.  (4, GEMM+LayerNorm, is not reported: ids 44, 45
   and 56 are the cases of csrc/igemm_ln.hip.)  Returns the number of configurations of the family (negative:
   unknown family).  With 0 <= index < that number and out != NULL, fills out[0..9]: families 0-3: id, BM, BN,
   BK, STAGES, WM, WN, KSPLIT, MT, bits (1 four-phase loop, 2 takes packed W2, 4 takes GEMM+GEGLU); family 5:
   id, TH, TW, BN, CK, WNG, 0... */
int mixdq_tile_config(int family, int index, int* out);

/* Tile id of the LDS-resident-halo kernel (csrc/iconv.hip) that mixdq_qconv2d_w8a8[_table] runs this
 * INT8 conv on when no tile is forced -- 90: 8 x 16 output pixels x 80 channels per workgroup, 91:
 * 8 x 8 x 80, 92: 16 x 16 x 80 (64-byte channel chunks), 93: 16 x 16 x 160 (K % 160 == 0; the choice from
 * batch 8 on) -- or 0 when the implicit-GEMM family runs it (not 3x3 / stride 1 / pad 1, C % 64 != 0,
 * H or W % 8 != 0).  Ids 90 .. 93 can be forced through bits 8..15 of `flags`.  This query answers for
 * int8 weights; mixdq_conv_halo_select_flags takes the launch's flags. */
int mixdq_conv_halo_select(int N, int H, int W, int C, int K, int R, int S, int stride, int pad);
/* The same for a launch with these `flags`: MIXDQ_FLAG_W4 asks for the packed-W4 instantiations (same
 * range and the same rule as int8 weights, except that K <= 16 output channels without 16 x 16 patches stay
 * on the implicit-GEMM family -- measured; forced ids 90 .. 93 still take them),
 * MIXDQ_FLAG_W2 answers 0 (no packed-W2 conv); the other bits are ignored.  Like the nine-argument query it
 * answers 0 for every width when MIXDQ_HALO_CONV=0 is set in the environment, and for MIXDQ_FLAG_W4 also when
 * MIXDQ_HALO_W4=0 is (the A/B switch that keeps only packed convs on the implicit-GEMM family): the answer is what
 * an unforced launch of this process does, from the same switches, each read once per process. */
int mixdq_conv_halo_select_flags(int N, int H, int W, int C, int K, int R, int S, int stride, int pad,
                                 int flags);

/* Introspection (tests): the table the GEMM + GEGLU epilogue of the large tiles looks GELU up in --
 * 2 x 0x4c00 uint16: f16 bits of gelu(g) for the FP16 gate g with bits (sign << 15) | magnitude,
 * magnitude < 0x4c00 (|g| < 16), positive half first -- copied to `out_device` (77 824 bytes). */
int mixdq_gelu_table(uint16_t* out_device, mixdq_stream_t stream);
/* The FP16 -> FP16 SiLU table the GroupNorm apply pass of LARGE launches looks SiLU up in (round 6; built on first use
 * by the specification itself, include/mixdq_math.h: same bits as the arithmetic): n_pos entries for y = +bits, then
 * n_neg for y = -bits; values outside take the arithmetic.  Builds the table if needed; copies it to out_device
 * (2 * (n_pos + n_neg) bytes) unless null.  No reference counterpart (stock nn.SiLU). */
int mixdq_silu_table(uint16_t* out_device_or_null, int* n_pos, int* n_neg, mixdq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MIXDQ_HIP_H_ */
