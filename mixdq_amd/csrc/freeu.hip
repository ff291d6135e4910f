// FreeU for gfx950: the skip's Fourier filter and the backbone scale of one up-block ResNet's (hidden, skip) pair in ONE
// launch (include/mixdq_hip.h mixdq_freeu_f16; arithmetic: include/mixdq_math.h mixdq_freeu_*).
// No reference counterpart (the reference leaves FreeU to diffusers' apply_freeu / fourier_filter).
//
// At the threshold diffusers always passes (1) the filter scales four frequencies of a plane: seven real sums
// S_t = sum x * w_t over the plane (w = 1, cos / sin along y, cos / sin along x, cos / sin of the sum of the angles) and
// the correction y = x + g * sum_t S_t w_t.  No FFT, no complex arithmetic, no device sin / cos: the four twiddles of a
// pixel come from a host-made [H + W, 2] table, the product frequency from two multiplies and two FMAs.
//
//   ownership    a workgroup of four waves owns one (image, channel octet) of the skip over the WHOLE plane: the sums
//                never leave it.  Lane l owns the pixels l, l + 256, ...: one 16-byte load is 8 channels of one pixel.
//   residency    freeu_kernel<PPL>, PPL = 1 / 2 / 4 / 8 / 16 pixels per lane: every load of the plane is issued before
//                the first use and the plane stays in registers (4 PPL VGPRs) between the sums and the correction: read
//                once, written once.  PPL = 0 is the route of planes beyond 256 * 16 pixels: the same lane-to-pixel map
//                as a loop, the plane read a second time (from L2) for the correction.  Both routes add in the same
//                order: the same bits.
//   reduction    56 partial sums per lane (8 channels x 7).  Within a wave a reduce-SCATTER: at ^32, ^16, ^8 a lane
//                sends one half of what it still holds and keeps the other (28 + 14 + 7 exchanges), after which the 8
//                lanes lane / 8 == c hold channel c's seven sums, finished by three butterfly steps on those seven (21):
//                70 exchanges where a butterfly on all 56 takes 336.  Across waves through 1.1 KB of LDS: 56 lanes add
//                the four waves' rows left to right and multiply by g, every lane reads the 56 products back as float4.
//   placement    consecutive workgroups are dealt round-robin to the 8 XCDs, and the 8 octets that share a 128-byte line
//                of a pixel would each pull that line into another XCD's L2.  Within every whole group of 64 work items
//                the index is transposed (8 x 8), so that the 8 octets of a line run on ONE XCD.
//   backbone     the hidden's scale runs as extra workgroups behind the skip's: a 16-byte stream, four vectors per lane
//                all loaded first, whose channel octet decides once whether the vector is scaled or copied.
//   stores       plain C++ vector stores.  No scratch (profiles/freeu_isa.txt).
#include "common.h"
#include "../../include/mixdq_math.h"

namespace mixdq {
namespace {

constexpr int kLanes = MIXDQ_FREEU_LANES;
constexpr int kWaves = kLanes / 64;
constexpr int kMaxPpl = MIXDQ_FREEU_MAX_PPL;
constexpr int kSums = 7;                        // per channel
constexpr int kAcc = 8 * kSums;                 // per lane: acc[c * 7 + t]
constexpr int kHidVecs = 4;                     // 16-byte vectors of a lane of the backbone stream
constexpr int kXcdGroup = kNumXCD * 8;          // work items whose index is transposed: 8 XCDs x the 8 octets of a line

// the seven basis values of pixel p
__device__ __forceinline__ void basis_of(const float2* __restrict__ tw, int p, int H, int W, float* w) {
  const int y = p / W, x = p - y * W;
  const float2 ty = tw[y], tx = tw[H + x];
  mixdq_freeu_basis(ty.x, ty.y, tx.x, tx.y, w);
}

__device__ __forceinline__ void accumulate8(float* acc, const Half8& px, const float* w) {
#pragma unroll
  for (int c = 0; c < 8; ++c) mixdq_freeu_accumulate(acc + c * kSums, half_at(px, c), w);
}

__device__ __forceinline__ Half8 apply8(const Half8& px, const float* G, const float* w) {
  uint32_t h[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) h[c] = half_bits(mixdq_freeu_apply(half_at(px, c), G + c * kSums, w));
  Half8 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o.w[e] = h[2 * e] | (h[2 * e + 1] << 16);
  return o;
}

// One step of the reduce-scatter over N values: the lane whose `bit` is clear keeps the lower half, the other the upper.
template <int N>
__device__ __forceinline__ void scatter_step(float* acc, int lane, int bit) {
  const bool up = (lane & bit) != 0;
#pragma unroll
  for (int i = 0; i < N / 2; ++i) {
    const float keep = up ? acc[i + N / 2] : acc[i];
    const float send = up ? acc[i] : acc[i + N / 2];
    acc[i] = MIXDQ_ADD_RN(keep, __shfl_xor(send, bit));
  }
}

template <int PPL>
__global__ __launch_bounds__(kLanes) void freeu_kernel(const Half8* __restrict__ hidden, const Half8* __restrict__ skip,
                                                       Half8* __restrict__ out_hidden, Half8* __restrict__ out_skip,
                                                       const float* __restrict__ table, int stage,
                                                       const float2* __restrict__ tw, int skip_blocks, int oct_s, int oct_h,
                                                       int H, int W, int64_t hid_vecs) {
  __shared__ float wave_sum[kWaves][kAcc];
  __shared__ __attribute__((aligned(16))) float total[kAcc];
  const int tid = threadIdx.x;
  const float b = table[2 * stage], s = table[2 * stage + 1];
  int work = blockIdx.x;

  if (work >= skip_blocks) {
    // ---- the backbone stream
    const int64_t v0 = (int64_t)(work - skip_blocks) * (kLanes * kHidVecs) + tid;
    Half8 v[kHidVecs];
#pragma unroll
    for (int j = 0; j < kHidVecs; ++j)
      if (v0 + kLanes * j < hid_vecs) v[j] = hidden[v0 + kLanes * j];
#pragma unroll
    for (int j = 0; j < kHidVecs; ++j) {
      const int64_t i = v0 + kLanes * j;
      if (i >= hid_vecs) continue;
      Half8 o = v[j];
      if (b != 1.0f && (int)(i % oct_h) < (oct_h >> 1)) {        // (b == 1: the hidden's own bits)
        uint32_t h[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) h[c] = half_bits(mixdq_freeu_backbone(half_at(v[j], c), b));
#pragma unroll
        for (int e = 0; e < 4; ++e) o.w[e] = h[2 * e] | (h[2 * e + 1] << 16);
      }
      out_hidden[i] = o;
    }
    return;
  }

  // ---- the skip: which (image, octet)
  const int group0 = work - work % kXcdGroup;
  if (group0 + kXcdGroup <= skip_blocks) {                        // a whole group: 8 x 8 transposed
    const int local = work - group0;
    static_assert(kNumXCD == 8, "the 8 x 8 transposition: low three bits <-> high three bits");
    work = group0 + ((local & 7) << 3) + (local >> 3);
  }
  const int img = work / oct_s, oct = work - img * oct_s;
  const int HW = H * W;
  const int64_t base = (int64_t)img * HW * oct_s + oct;           // pixel p of the octet: vector base + p * oct_s
  const Half8* __restrict__ src = skip + base;
  Half8* __restrict__ dst = out_skip + base;

  if (s == 1.0f) {                                                // the skip's own bits
    for (int p = tid; p < HW; p += kLanes) dst[(int64_t)p * oct_s] = src[(int64_t)p * oct_s];
    return;
  }

  // ---- the sums of this lane's pixels
  float acc[kAcc];
#pragma unroll
  for (int i = 0; i < kAcc; ++i) acc[i] = 0.0f;
  Half8 px[PPL > 0 ? PPL : 1];
  if constexpr (PPL > 0) {
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int p = tid + kLanes * j;
      if (p < HW) px[j] = src[(int64_t)p * oct_s];
    }
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int p = tid + kLanes * j;
      if (p < HW) {
        float w[kSums];
        basis_of(tw, p, H, W, w);
        accumulate8(acc, px[j], w);
      }
    }
  } else {
    for (int p = tid; p < HW; p += kLanes) {
      float w[kSums];
      basis_of(tw, p, H, W, w);
      accumulate8(acc, src[(int64_t)p * oct_s], w);
    }
  }

  // ---- over the wave: reduce-scatter to one channel per 8 lanes, then a butterfly on its seven sums
  const int lane = tid & 63, wave = tid >> 6;
  scatter_step<56>(acc, lane, 32);
  scatter_step<28>(acc, lane, 16);
  scatter_step<14>(acc, lane, 8);
#pragma unroll
  for (int bit = 4; bit >= 1; bit >>= 1)
#pragma unroll
    for (int t = 0; t < kSums; ++t) acc[t] = MIXDQ_ADD_RN(acc[t], __shfl_xor(acc[t], bit));
  if ((lane & 7) == 0) {
#pragma unroll
    for (int t = 0; t < kSums; ++t) wave_sum[wave][(lane >> 3) * kSums + t] = acc[t];
  }
  __syncthreads();
  // ---- over the waves, left to right, times g
  if (tid < kAcc) {
    float t = wave_sum[0][tid];
#pragma unroll
    for (int wv = 1; wv < kWaves; ++wv) t = MIXDQ_ADD_RN(t, wave_sum[wv][tid]);
    total[tid] = MIXDQ_MUL_RN(mixdq_freeu_gain(s, (int64_t)HW), t);
  }
  __syncthreads();
  float G[kAcc];
#pragma unroll
  for (int i = 0; i < kAcc / 4; ++i) {
    const float4 q = *reinterpret_cast<const float4*>(total + 4 * i);
    G[4 * i] = q.x, G[4 * i + 1] = q.y, G[4 * i + 2] = q.z, G[4 * i + 3] = q.w;
  }

  // ---- the correction, one rounding to FP16
  if constexpr (PPL > 0) {
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int p = tid + kLanes * j;
      if (p < HW) {
        float w[kSums];
        basis_of(tw, p, H, W, w);
        dst[(int64_t)p * oct_s] = apply8(px[j], G, w);
      }
    }
  } else {
    for (int p = tid; p < HW; p += kLanes) {
      float w[kSums];
      basis_of(tw, p, H, W, w);
      dst[(int64_t)p * oct_s] = apply8(src[(int64_t)p * oct_s], G, w);
    }
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

constexpr int64_t kMaxGrid = 0x7fffffff;

}  // namespace
}  // namespace mixdq

using namespace mixdq;

extern "C" int mixdq_freeu_resident_pixels(void) { return kLanes * kMaxPpl; }

extern "C" int mixdq_freeu_f16(const void* hidden, const void* skip, void* out_hidden, void* out_skip, const float* table,
                               int stage, const float* twiddles, int B, int C_h, int C_s, int H, int W,
                               mixdq_stream_t stream_) {
  if (!hidden || !skip || !out_hidden || !out_skip || !table || !twiddles) return MIXDQ_ERR_INVALID_ARG;
  if (stage < 0 || stage > 1 || B < 0 || C_h < 0 || C_s < 0 || H < 0 || W < 0) return MIXDQ_ERR_INVALID_ARG;
  if (H < 2 || W < 2 || C_s % 8 != 0 || C_h % 16 != 0) return MIXDQ_ERR_SHAPE;
  const int64_t HW = (int64_t)H * W;
  if (HW > kMaxGrid - kLanes) return MIXDQ_ERR_INVALID_ARG;       // (a lane's pixel index is an int)
  const int64_t n_h = (int64_t)B * HW * C_h * 2, n_s = (int64_t)B * HW * C_s * 2;      // bytes
  if (overlap(out_hidden, n_h, hidden, n_h) || overlap(out_hidden, n_h, skip, n_s) || overlap(out_skip, n_s, skip, n_s) ||
      overlap(out_skip, n_s, hidden, n_h) || overlap(out_skip, n_s, out_hidden, n_h))
    return MIXDQ_ERR_INVALID_ARG;
  if (!aligned(hidden, 16) || !aligned(skip, 16) || !aligned(out_hidden, 16) || !aligned(out_skip, 16) ||
      !aligned(twiddles, 8) || !aligned(table, 4))
    return MIXDQ_ERR_ALIGNMENT;
  const int oct_s = C_s / 8, oct_h = C_h / 8;
  const int64_t skip_blocks = (int64_t)B * oct_s;
  const int64_t hid_vecs = (int64_t)B * HW * oct_h;
  const int64_t blocks = skip_blocks + (hid_vecs + kLanes * kHidVecs - 1) / (kLanes * kHidVecs);
  if (blocks > kMaxGrid) return MIXDQ_ERR_INVALID_ARG;
  if (blocks == 0) return MIXDQ_OK;
  // the smallest instantiation that holds the plane; 0: the plane is read twice
  int ppl = 0;
  for (int c = kMaxPpl; c >= 1; c >>= 1)
    if (HW <= (int64_t)kLanes * c) ppl = c;
  hipStream_t stream = (hipStream_t)stream_;
  with_constant<0, 1, 2, 4, 8, 16>(ppl, [&](auto c) {
    freeu_kernel<decltype(c)::value><<<(unsigned)blocks, kLanes, 0, stream>>>(
        (const Half8*)hidden, (const Half8*)skip, (Half8*)out_hidden, (Half8*)out_skip, table, stage,
        (const float2*)twiddles, (int)skip_blocks, oct_s, oct_h, H, W, hid_vecs);
  });
  return launch_status();
}
