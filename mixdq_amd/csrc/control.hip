// ControlNet glue for gfx950: the three launches a ControlNet needs beside the UNet's own.  No reference counterpart
// (the reference passes down_block_additional_residuals / mid_block_additional_residual through to diffusers).
//
//   mixdq_control_add_f16      every skip tensor of a UNet (the mid-block output included) plus the scaled residuals of
//                              up to 4 nets, ONE launch; the scales come from a device table indexed by the device-side
//                              step counter, so a captured graph serves every scale and guidance window
//   mixdq_silu_f16             a stand-alone SiLU (the activation between the hint convs)
//   mixdq_hint_to_nhwc8_f16    the hint image ingest, [0, 1] rule
//
// Arithmetic: include/mixdq_math.h (mixdq_control_scaled / mixdq_control_sum, mixdq_siluf, mixdq_hint_unit), every
// FP16 rounding through f32_to_f16_rn.
//
// All three grids are EXACT: one workgroup of 256 lanes per fixed chunk, no grid-stride loop, no cap.
//
// mixdq_control_add_f16 streams: 2 x (1 + K) 16-byte loads per lane, all issued before the first use (the skip's
// first: they do not wait for the scale), two 16-byte stores.  The segment descriptors -- 16 x 6 pointers, the element
// counts, the first workgroup of every segment -- are kernel arguments BY VALUE (under 1 KB): a captured graph carries
// them in its kernel node, no pointer table is copied to the device.  A workgroup finds its segment as the last
// one that starts at or below its index: 15 scalar compares and selects on values that arrive with the first wait.
#include "common.h"
#include "../../include/mixdq_math.h"

namespace mixdq {
namespace {

constexpr int kChunk = 4096;                    // FP16 elements of a workgroup: 256 lanes x 2 vectors of 8
constexpr int kVecs = kChunk / 8 / 256;         // 16-byte vectors of a lane
constexpr int kMaxSeg = MIXDQ_CONTROL_MAX_SEGMENTS;
constexpr int kMaxNets = MIXDQ_CONTROL_MAX_NETS;

struct ControlAddArgs {
  uint32_t first[kMaxSeg];                      // first[i]: the first workgroup of segment i (i >= S: the total)
  const float* scales;                          // [K, n_steps]
  const int* step;
  int n_steps;
  int pad_;
  int64_t n[kMaxSeg];
  const Half8* skip[kMaxSeg];
  Half8* dst[kMaxSeg];
  const Half8* res[kMaxNets][kMaxSeg];
};
static_assert(sizeof(ControlAddArgs) < 1024, "the descriptors travel in the kernel arguments");

// The step counter and the scale table are read through the constant address space: scalar loads (the same value in
// every lane, no vector-memory round trip in front of the residuals' loads).  Both were written by EARLIER kernels of the
// stream -- the sampler's advance, a host copy -- never by this one.
typedef const int __attribute__((address_space(4))) * ScalarIntPtr;
typedef const float __attribute__((address_space(4))) * ScalarFloatPtr;
__device__ __forceinline__ int scalar_load(const int* p) { return *(ScalarIntPtr)(uintptr_t)p; }
__device__ __forceinline__ float scalar_load(const float* p) { return *(ScalarFloatPtr)(uintptr_t)p; }

// an FP32 value rounded to FP16, as the FP32 value the next operation reads
__device__ __forceinline__ float via_f16(float v) { return __half2float(f32_to_f16_rn(v)); }

template <int K>
__global__ __launch_bounds__(256) void control_add_kernel(const ControlAddArgs a) {
  MIXDQ_ARGS_NOW(a.scales, a.step, a.n_steps);        // with the segment starts, behind one wait: the step is read next
  const int st = scalar_load(a.step);
  const uint32_t bid = blockIdx.x;
  int seg = 0;
#pragma unroll
  for (int i = 1; i < kMaxSeg; ++i) seg = a.first[i] <= bid ? i : seg;      // (an empty segment starts where the next does)
  const int64_t nv = a.n[seg] >> 3;                                          // 16-byte vectors of the segment
  const int64_t v0 = (int64_t)(bid - a.first[seg]) * (kChunk / 8) + (int)threadIdx.x;
  const Half8* skip = a.skip[seg];
  Half8* dst = a.dst[seg];
  bool ok[kVecs];
  Half8 sk[kVecs];
#pragma unroll
  for (int j = 0; j < kVecs; ++j) {
    ok[j] = v0 + 256 * j < nv;
    if (ok[j]) sk[j] = skip[v0 + 256 * j];
  }
  // the scales of this step: the same in every lane, held in scalar registers; a step outside the table: all zero
  const bool in_table = st >= 0 && st < a.n_steps;
  float s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    s[k] = in_table ? scalar_load(a.scales + ((int64_t)k * a.n_steps + st)) : 0.0f;
  }
  Half8 r[K][kVecs];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (s[k] != 0.0f) {                                                      // (a closed window: not loaded)
      const Half8* res = a.res[k][seg];
#pragma unroll
      for (int j = 0; j < kVecs; ++j)
        if (ok[j]) r[k][j] = res[v0 + 256 * j];
    }
  }
#pragma unroll
  for (int j = 0; j < kVecs; ++j) {
    if (!ok[j]) continue;
    Half8 o = sk[j];
    bool any = false;
    float acc[8];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (s[k] == 0.0f) continue;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float t = via_f16(mixdq_control_scaled(half_at(r[k][j], e), s[k]));
        acc[e] = any ? via_f16(mixdq_control_sum(acc[e], t)) : t;
      }
      any = true;
    }
    if (any) {
      uint32_t h[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = half_bits(mixdq_control_sum(half_at(sk[j], e), acc[e]));
#pragma unroll
      for (int e = 0; e < 4; ++e) o.w[e] = h[2 * e] | (h[2 * e + 1] << 16);
    }
    dst[v0 + 256 * j] = o;                                                   // (every net skipped: the skip's own bits)
  }
}

constexpr int kSiluSpan = 2048;                 // FP16 elements of a workgroup: one 16-byte vector per lane

__global__ __launch_bounds__(256) void silu_f16_kernel(const Half8* x, Half8* out, int64_t nv) {
  const int64_t v = (int64_t)blockIdx.x * 256 + (int)threadIdx.x;
  if (v >= nv) return;
  const Half8 in = x[v];
  uint32_t h[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) h[e] = half_bits(mixdq_siluf(half_at(in, e)));
  Half8 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o.w[e] = h[2 * e] | (h[2 * e + 1] << 16);
  out[v] = o;
}

// one source element as the FP32 value that is rounded to FP16
__device__ __forceinline__ float hint_value(uint8_t u) { return mixdq_hint_unit((uint32_t)u); }
__device__ __forceinline__ float hint_value(__half h) { return __half2float(h); }
__device__ __forceinline__ float hint_value(float f) { return f; }

// One lane = one pixel: up to 8 strided element loads, one 16-byte store.
template <typename T>
__global__ __launch_bounds__(256) void hint_to_nhwc8_kernel(const T* __restrict__ img, int64_t sb, int64_t sc, int64_t sh,
                                                            int64_t sw, Half8* __restrict__ out, int64_t pixels, int C,
                                                            int H, int W) {
  const int64_t i = (int64_t)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= pixels) return;
  const int64_t row = i / W;
  const int x = (int)(i - row * W);
  const int64_t b = row / H;
  const int y = (int)(row - b * H);
  const T* px = img + (b * sb + y * sh + x * sw);
  T v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = c < C ? px[c * sc] : T(0);              // channels >= C are never read
  uint32_t h[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) h[c] = c < C ? half_bits(hint_value(v[c])) : 0u;
  Half8 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o.w[j] = h[2 * j] | (h[2 * j + 1] << 16);
  out[i] = o;
}

constexpr int64_t kMaxGrid = 0x7fffffff;        // the x extent of a grid

}  // namespace
}  // namespace mixdq

using namespace mixdq;

extern "C" int mixdq_control_chunk(void) { return kChunk; }

extern "C" int mixdq_control_add_f16(const void* const* skip, void* const* dst, const void* const* residuals,
                                     const int64_t* n, int S, int K, const float* scales, int n_steps, const int* step,
                                     mixdq_stream_t stream_) {
  if (S < 1 || S > kMaxSeg || K < 1 || K > kMaxNets || n_steps < 1) return MIXDQ_ERR_INVALID_ARG;
  if (!skip || !dst || !residuals || !n || !scales || !step) return MIXDQ_ERR_INVALID_ARG;
  ControlAddArgs a = {};
  int64_t blocks = 0;
  bool misaligned = (uintptr_t)scales % 4 || (uintptr_t)step % 4;
  for (int i = 0; i < S; ++i) {
    if (n[i] < 0) return MIXDQ_ERR_INVALID_ARG;
    a.first[i] = (uint32_t)blocks;
    a.n[i] = n[i];
    if (n[i] == 0) continue;                          // (an empty tensor has no storage: its pointers are not looked at)
    misaligned |= n[i] % 8 != 0;
    if (!skip[i] || !dst[i]) return MIXDQ_ERR_INVALID_ARG;
    misaligned |= (uintptr_t)skip[i] % 16 || (uintptr_t)dst[i] % 16;
    a.skip[i] = (const Half8*)skip[i];
    a.dst[i] = (Half8*)dst[i];
    for (int k = 0; k < K; ++k) {
      const void* r = residuals[(size_t)k * S + i];
      if (!r) return MIXDQ_ERR_INVALID_ARG;
      misaligned |= (uintptr_t)r % 16 != 0;
      a.res[k][i] = (const Half8*)r;
    }
    blocks += (n[i] + kChunk - 1) / kChunk;
    if (blocks > kMaxGrid) return MIXDQ_ERR_INVALID_ARG;
  }
  if (misaligned) return MIXDQ_ERR_ALIGNMENT;
  for (int i = S; i < kMaxSeg; ++i) a.first[i] = (uint32_t)blocks;
  if (blocks == 0) return MIXDQ_OK;
  a.scales = scales;
  a.step = step;
  a.n_steps = n_steps;
  hipStream_t stream = (hipStream_t)stream_;
  with_constant<1, 2, 3, 4>(K, [&](auto k) {
    control_add_kernel<decltype(k)::value><<<(unsigned)blocks, 256, 0, stream>>>(a);
  });
  return launch_status();
}

extern "C" int mixdq_silu_f16(const void* x_f16, void* out_f16, int64_t n, mixdq_stream_t stream_) {
  if (n < 0) return MIXDQ_ERR_INVALID_ARG;
  if (n == 0) return MIXDQ_OK;                        // (an empty tensor has no storage: before the pointer checks)
  if (!x_f16 || !out_f16) return MIXDQ_ERR_INVALID_ARG;
  const int64_t blocks = (n + kSiluSpan - 1) / kSiluSpan;
  if (blocks > kMaxGrid) return MIXDQ_ERR_INVALID_ARG;
  if (n % 8 || (uintptr_t)x_f16 % 16 || (uintptr_t)out_f16 % 16) return MIXDQ_ERR_ALIGNMENT;
  silu_f16_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream_>>>((const Half8*)x_f16, (Half8*)out_f16, n >> 3);
  return launch_status();
}

extern "C" int mixdq_hint_to_nhwc8_f16(const void* img, int dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                                       void* out_f16, int B, int C, int H, int W, mixdq_stream_t stream_) {
  const int elem = image_elem_size(dtype);
  if (B < 0 || H < 0 || W < 0 || C < 1 || C > 8 || !elem) return MIXDQ_ERR_INVALID_ARG;
  const int64_t pixels = (int64_t)B * H * W;
  if (pixels == 0) return MIXDQ_OK;                   // (an empty tensor has no storage: before the pointer checks)
  if (!img || !out_f16) return MIXDQ_ERR_INVALID_ARG;
  const int64_t blocks = (pixels + 255) / 256;
  if (blocks > kMaxGrid) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)out_f16 % 16 || (uintptr_t)img % elem) return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  Half8* out = (Half8*)out_f16;
  with_image_type(dtype, [&](auto t) {
    using T = decltype(t);
    hint_to_nhwc8_kernel<T><<<(unsigned)blocks, 256, 0, stream>>>((const T*)img, sb, sc, sh, sw, out, pixels, C, H, W);
  });
  return launch_status();
}
