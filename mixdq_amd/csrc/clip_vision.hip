// The front of a CLIP vision tower in ONE launch: image normalisation, the 14 x 14 / stride-14 patch convolution, the
// class token, the position embedding and pre_layrnorm -- raw image in, the first transformer layer's input out
// (include/mixdq_hip.h mixdq_clip_patch_embed_f16; arithmetic: include/mixdq_math.h mixdq_clip_*).
//
// A kernel of its own, not a member of the conv family: C = 3 and K = 588 fit none of its tiles, and the rows of the
// product are LayerNorm rows.
//
//   ownership    a workgroup of four waves owns kRows = 16 consecutive patches over ALL N columns: the row statistics of
//                the LayerNorm never leave it.  Grid (ceil(g^2 / 16) + 1, B): the last block in x owns the class-token
//                row of its image and runs no product.
//   ingest       the 256 lanes gather the block's 16 x 588 pixels from the strided image (consecutive lanes walk along
//                an image row across neighbouring patches), normalise them and store FP16 im2col rows [16][kPitch] in
//                LDS (19.25 KB); taps 588 .. 607 and patches past g^2 are zeros.  One barrier.
//   orientation  D[i, j] = sum_k W[n0 + i, k] * pix[j, k] on v_mfma_f32_16x16x32_f16: the MFMA's row index i is an
//                output COLUMN, its column index j a PATCH, so the four accumulator registers of a lane are four
//                consecutive columns of one token -- pos loads and output stores are 8-byte pieces, and a row's
//                statistics need two lane exchanges and one LDS round.
//   operands     the pixel fragments come from LDS (all four waves read the same ones; kPitch = 616 halves puts the 16
//                rows of a 16-byte read into 16 different bank groups); the weight fragments go straight from global
//                memory into registers, 16 bytes per lane, tile and K-step, one K-step ahead of the MFMAs that use them.
//                A wave owns N / 4 columns and no other wave reads its weight rows; across workgroups the 1.5 MB of
//                weights stay in L2.
//   epilogue     in registers: round, add pos, (two-pass LayerNorm), store.  No scratch.
#include "common.h"
#include "../../include/mixdq_math.h"

namespace mixdq {
namespace {

constexpr int kRows = 16;                    // patches per workgroup
constexpr int kPatch = MIXDQ_CLIP_PATCH;     // 14
constexpr int kTaps = 3 * kPatch * kPatch;   // 588
constexpr int kKp = MIXDQ_CLIP_KP;           // 608 = 19 x 32
constexpr int kSteps = kKp / 32;             // 19
constexpr int kPitch = kKp + 8;              // halves per im2col row: 1232 bytes = 77 x 16, 77 odd
constexpr int kLine = kRows * kPatch;        // 224 pixels: one image row of the block's patches

__device__ __forceinline__ float pixel_of(const uint8_t* p) { return (float)*p; }
__device__ __forceinline__ float pixel_of(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ float pixel_of(const float* p) { return *p; }

__device__ __forceinline__ float half_value(uint32_t bits) {
  __half_raw r;
  r.x = (unsigned short)(bits & 0xffffu);
  return __half2float(__half(r));
}

// The block's im2col rows: item = (c * 14 + y) * 224 + (patch * 14 + x), so that consecutive lanes read along an image row.
template <class T>
__device__ __forceinline__ void ingest(const T* __restrict__ img, int64_t sc, int64_t sh, int64_t sw,
                                       const float* __restrict__ norm, int g, int patches, int p0,
                                       unsigned short* __restrict__ rows, int tid) {
  float na[3], nb[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) na[c] = norm[2 * c], nb[c] = norm[2 * c + 1];
  // (eight gathers in flight per lane were measured: no faster -- the launch is bound by the weight stream)
  for (int idx = tid; idx < 3 * kPatch * kLine; idx += 256) {
    const int cy = idx / kLine, r = idx - cy * kLine;
    const int pi = r / kPatch, x = r - pi * kPatch;
    const int c = cy / kPatch, y = cy - c * kPatch;
    const int p = p0 + pi;
    unsigned short v = 0;
    if (p < patches) {
      const int py = p / g, px = p - py * g;
      const float u = pixel_of(img + c * sc + (int64_t)(py * kPatch + y) * sh + (int64_t)(px * kPatch + x) * sw);
      const float a = c == 0 ? na[0] : c == 1 ? na[1] : na[2], b = c == 0 ? nb[0] : c == 1 ? nb[1] : nb[2];
      v = (unsigned short)half_bits(mixdq_clip_pixel(u, a, b));
    }
    rows[pi * kPitch + cy * kPatch + x] = v;
  }
  for (int idx = tid; idx < kRows * (kKp - kTaps); idx += 256) {
    const int pi = idx / (kKp - kTaps);
    rows[pi * kPitch + kTaps + (idx - pi * (kKp - kTaps))] = 0;
  }
}

// MAXT: the accumulator tiles a wave has registers for; nt = N / 64 <= MAXT of them are real.
template <int MAXT>
__global__ __launch_bounds__(256) void clip_patch_embed_kernel(
    const void* __restrict__ image, int dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
    const float* __restrict__ norm, const _Float16* __restrict__ weight, const unsigned short* __restrict__ cls,
    const unsigned short* __restrict__ pos, const unsigned short* __restrict__ ln_w,
    const unsigned short* __restrict__ ln_b, float eps, unsigned short* __restrict__ out, int64_t ldo, int g, int N) {
  __shared__ __attribute__((aligned(16))) unsigned short rows[kRows * kPitch];
  __shared__ float red[2][4][kRows];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, tk = lane & 15, q = lane >> 4;
  const int patches = g * g, nt = N >> 6, b = blockIdx.y;
  const bool is_cls = (int)blockIdx.x * kRows >= patches;       // the one block past the patch blocks
  const int p = blockIdx.x * kRows + tk;                        // this lane's patch
  const int col0 = wave * (N >> 2) + q * 4;                     // + 16 t + e: this lane's columns
  const bool row_ok = is_cls ? tk == 0 : p < patches;
  const int row = is_cls ? 0 : 1 + p;                           // the token
  const unsigned short* prow = pos + (int64_t)(row_ok ? row : 0) * N + col0;

  v4f acc[MAXT];
  if (is_cls) {
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      acc[t] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
      if (t < nt) {
        const uint2 c = *reinterpret_cast<const uint2*>(cls + col0 + t * 16);
        const uint2 o = *reinterpret_cast<const uint2*>(prow + t * 16);
        acc[t][0] = half_value(half_bits(mixdq_clip_embed(half_value(c.x), half_value(o.x))));
        acc[t][1] = half_value(half_bits(mixdq_clip_embed(half_value(c.x >> 16), half_value(o.x >> 16))));
        acc[t][2] = half_value(half_bits(mixdq_clip_embed(half_value(c.y), half_value(o.y))));
        acc[t][3] = half_value(half_bits(mixdq_clip_embed(half_value(c.y >> 16), half_value(o.y >> 16))));
      }
    }
  } else {
    // ---- ingest
    const int64_t img_off = (int64_t)b * sb;
    if (dtype == MIXDQ_IMAGE_U8)
      ingest((const uint8_t*)image + img_off, sc, sh, sw, norm, g, patches, blockIdx.x * kRows, rows, tid);
    else if (dtype == MIXDQ_IMAGE_F16)
      ingest((const __half*)image + img_off, sc, sh, sw, norm, g, patches, blockIdx.x * kRows, rows, tid);
    else
      ingest((const float*)image + img_off, sc, sh, sw, norm, g, patches, blockIdx.x * kRows, rows, tid);

    // ---- the product.  A tile past nt reads the last real tile's weights again and its result is dropped.
    // (the tile's base is uniform -- scalar registers -- and the lane's offset one 32-bit value for every load)
    const _Float16* wbase = weight + (int64_t)__builtin_amdgcn_readfirstlane(wave) * (N >> 2) * kKp;
    const int loff = tk * kKp + q * 8;
    auto wfrag = [&](int t, int ks) {
      const int tt = t < nt ? t : nt - 1;
      return *reinterpret_cast<const v8h*>(wbase + tt * (16 * kKp) + ks * 32 + loff);
    };
    v8h wf[2][MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      wf[0][t] = wfrag(t, 0);
      acc[t] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    }
    __syncthreads();
    const unsigned short* xrow = rows + tk * kPitch + q * 8;
#pragma unroll
    for (int ks = 0; ks < kSteps; ++ks) {
      if (ks + 1 < kSteps) {
#pragma unroll
        for (int t = 0; t < MAXT; ++t) wf[(ks + 1) & 1][t] = wfrag(t, ks + 1);
      }
      const v8h x = *reinterpret_cast<const v8h*>(xrow + ks * 32);
#pragma unroll
      for (int t = 0; t < MAXT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[ks & 1][t], x, acc[t], 0, 0, 0);
    }
    // ---- e = f16(f16(acc) + pos)
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      if (t < nt && row_ok) {
        const uint2 o = *reinterpret_cast<const uint2*>(prow + t * 16);
        acc[t][0] = half_value(half_bits(mixdq_clip_embed(half_value(half_bits(acc[t][0])), half_value(o.x))));
        acc[t][1] = half_value(half_bits(mixdq_clip_embed(half_value(half_bits(acc[t][1])), half_value(o.x >> 16))));
        acc[t][2] = half_value(half_bits(mixdq_clip_embed(half_value(half_bits(acc[t][2])), half_value(o.y))));
        acc[t][3] = half_value(half_bits(mixdq_clip_embed(half_value(half_bits(acc[t][3])), half_value(o.y >> 16))));
      }
    }
  }

  unsigned short* orow = out + ((int64_t)b * (patches + 1) + (row_ok ? row : 0)) * ldo + col0;
  if (ln_w == nullptr) {
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
      if (t < nt && row_ok)
        *reinterpret_cast<uint2*>(orow + t * 16) = make_uint2(half_bits(acc[t][0]) | (half_bits(acc[t][1]) << 16),
                                                              half_bits(acc[t][2]) | (half_bits(acc[t][3]) << 16));
    return;
  }

  // ---- LayerNorm over the row: two passes, lanes -> lane groups -> waves, in a fixed order
  float s = 0.0f;
#pragma unroll
  for (int t = 0; t < MAXT; ++t)
    if (t < nt) {
#pragma unroll
      for (int e = 0; e < 4; ++e) s = MIXDQ_ADD_RN(s, acc[t][e]);
    }
  s = MIXDQ_ADD_RN(s, __shfl_xor(s, 16));
  s = MIXDQ_ADD_RN(s, __shfl_xor(s, 32));
  if (q == 0) red[0][wave][tk] = s;
  __syncthreads();
  const float mean = mixdq_clip_ln_mean(
      MIXDQ_ADD_RN(MIXDQ_ADD_RN(MIXDQ_ADD_RN(red[0][0][tk], red[0][1][tk]), red[0][2][tk]), red[0][3][tk]), N);
  float ss = 0.0f;
#pragma unroll
  for (int t = 0; t < MAXT; ++t)
    if (t < nt) {
#pragma unroll
      for (int e = 0; e < 4; ++e) ss = mixdq_clip_ln_sq(acc[t][e], mean, ss);
    }
  ss = MIXDQ_ADD_RN(ss, __shfl_xor(ss, 16));
  ss = MIXDQ_ADD_RN(ss, __shfl_xor(ss, 32));
  if (q == 0) red[1][wave][tk] = ss;
  __syncthreads();
  const float rstd = mixdq_clip_ln_rstd(
      MIXDQ_ADD_RN(MIXDQ_ADD_RN(MIXDQ_ADD_RN(red[1][0][tk], red[1][1][tk]), red[1][2][tk]), red[1][3][tk]), N, eps);
  if (!row_ok) return;
#pragma unroll
  for (int t = 0; t < MAXT; ++t)
    if (t < nt) {
      const uint2 gm = *reinterpret_cast<const uint2*>(ln_w + col0 + t * 16);
      const uint2 bt = *reinterpret_cast<const uint2*>(ln_b + col0 + t * 16);
      const uint32_t y0 = half_bits(mixdq_clip_ln_apply(acc[t][0], mean, rstd, half_value(gm.x), half_value(bt.x)));
      const uint32_t y1 = half_bits(mixdq_clip_ln_apply(acc[t][1], mean, rstd, half_value(gm.x >> 16), half_value(bt.x >> 16)));
      const uint32_t y2 = half_bits(mixdq_clip_ln_apply(acc[t][2], mean, rstd, half_value(gm.y), half_value(bt.y)));
      const uint32_t y3 = half_bits(mixdq_clip_ln_apply(acc[t][3], mean, rstd, half_value(gm.y >> 16), half_value(bt.y >> 16)));
      *reinterpret_cast<uint2*>(orow + t * 16) = make_uint2(y0 | (y1 << 16), y2 | (y3 << 16));
    }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace
}  // namespace mixdq

extern "C" int mixdq_clip_patch_embed_f16(const void* image, int dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                                          const float* norm, const void* weight_f16, const void* cls_f16,
                                          const void* pos_f16, int pos_rows, const void* ln_weight_f16,
                                          const void* ln_bias_f16, float eps, void* out_f16, int64_t ldo, int B, int S,
                                          int N, mixdq_stream_t stream) {
  using namespace mixdq;
  if (!image || !norm || !weight_f16 || !cls_f16 || !pos_f16 || !out_f16 || B < 0 || B > 65535 ||
      image_elem_size(dtype) == 0 || (ln_weight_f16 == nullptr) != (ln_bias_f16 == nullptr))
    return MIXDQ_ERR_INVALID_ARG;
  if (S < kPatch || S % kPatch != 0 || S / kPatch > MIXDQ_CLIP_MAX_GRID || N < 64 || N % 64 != 0 || N > MIXDQ_CLIP_MAX_N)
    return MIXDQ_ERR_SHAPE;
  const int g = S / kPatch;
  if (pos_rows != g * g + 1 || ldo < N || ldo % 4 != 0) return MIXDQ_ERR_SHAPE;
  if (!aligned(image, image_elem_size(dtype)) || !aligned(norm, 4) || !aligned(weight_f16, 16) || !aligned(cls_f16, 8) ||
      !aligned(pos_f16, 8) || !aligned(ln_weight_f16, 8) || !aligned(ln_bias_f16, 8) || !aligned(out_f16, 8))
    return MIXDQ_ERR_ALIGNMENT;
  if (B == 0) return MIXDQ_OK;
  const dim3 grid((unsigned)((g * g + kRows - 1) / kRows + 1), (unsigned)B);
  const int nt = N / 64;
  const int maxt = nt <= 4 ? 4 : nt <= 12 ? 12 : nt <= 16 ? 16 : nt <= 20 ? 20 : 32;
  with_constant<4, 12, 16, 20, 32>(maxt, [&](auto T) {
    hipLaunchKernelGGL(clip_patch_embed_kernel<decltype(T)::value>, grid, dim3(256), 0, (hipStream_t)stream, image, dtype,
                       sb, sc, sh, sw, norm, (const _Float16*)weight_f16, (const unsigned short*)cls_f16,
                       (const unsigned short*)pos_f16, (const unsigned short*)ln_weight_f16,
                       (const unsigned short*)ln_bias_f16, eps, (unsigned short*)out_f16, ldo, g, N);
  });
  return launch_status();
}
