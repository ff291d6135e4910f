// The two ends of the VAE encoder for gfx950: the image ingest in front of conv_in and the posterior sample behind
// quant_conv.  No reference counterpart: the reference reaches the VAE only through diffusers' pipeline.
//
//   mixdq_image_to_nhwc8_f16   [B, C <= 8, H, W] uint8 / FP16 / FP32 at any element strides -> FP16 [B, H, W, 8],
//                              channels C..7 zero: the 8-channel form conv_in takes on the MFMA tiles (2C % 16 == 0)
//   mixdq_vae_latent_sample    FP16 moments [B, h, w, 2L] (+ FP32 noise [B, h, w, L]) -> FP32 z [B, h, w, L]
//
// Arithmetic: include/mixdq_math.h (mixdq_pixel_to_unit, mixdq_vae_latent[_mode]), FP32 round-to-nearest, never
// contracted.  Both are HBM-bound and grid-stride, one pixel (one group of four latent channels) per lane per trip;
// every load of a trip is requested before the first value is used, and each lane writes one 16-byte store.
#include "common.h"
#include "../../include/mixdq_math.h"

namespace mixdq {
namespace {

struct alignas(16) Half8 { uint32_t w[4]; };
struct alignas(8) Half4 { uint32_t w[2]; };

__device__ __forceinline__ float half_of(uint32_t word, int hi) {
  __half_raw hr;
  hr.x = (unsigned short)(hi ? (word >> 16) : (word & 0xffffu));
  return __half2float(__half(hr));
}

__device__ __forceinline__ uint32_t half_bits(float v) {
  return (uint32_t)__half_raw(f32_to_f16_rn(v)).x;
}

// one source element as the FP32 value that is rounded to FP16
__device__ __forceinline__ float ingest_value(uint8_t u) { return mixdq_pixel_to_unit((uint32_t)u); }
__device__ __forceinline__ float ingest_value(__half h) { return __half2float(h); }
__device__ __forceinline__ float ingest_value(float f) { return f; }

template <typename T>
__global__ __launch_bounds__(256) void image_to_nhwc8_kernel(const T* __restrict__ img, int64_t sb, int64_t sc,
                                                             int64_t sh, int64_t sw, Half8* __restrict__ out,
                                                             int64_t pixels, int C, int H, int W) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += stride) {
    const int64_t row = i / W;
    const int x = (int)(i - row * W);
    const int64_t b = row / H;
    const int y = (int)(row - b * H);
    const T* px = img + (b * sb + y * sh + x * sw);
    T v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = c < C ? px[c * sc] : T(0);     // channels >= C are never read
    uint32_t h[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) h[c] = c < C ? half_bits(ingest_value(v[c])) : 0u;
    Half8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o.w[j] = h[2 * j] | (h[2 * j + 1] << 16);
    out[i] = o;
  }
}

// One lane = four latent channels of one pixel.  L4: a pixel's moments are one 16-byte row (mean | logvar).
template <bool NOISE, bool L4>
__global__ __launch_bounds__(256) void vae_latent_kernel(const __half* __restrict__ moments,
                                                         const float* __restrict__ noise, float* __restrict__ z,
                                                         int64_t groups, int L, float sf) {
  const int gpp = L >> 2;                            // groups per pixel
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += stride) {
    Half4 mean, logvar = {{0u, 0u}};
    if constexpr (L4) {
      const Half8 m = *reinterpret_cast<const Half8*>(moments + i * 8);
      mean.w[0] = m.w[0]; mean.w[1] = m.w[1];
      logvar.w[0] = m.w[2]; logvar.w[1] = m.w[3];
    } else {
      const int64_t pixel = i / gpp;
      const int g = (int)(i - pixel * gpp);
      const __half* row = moments + pixel * (2 * (int64_t)L) + 4 * g;
      mean = *reinterpret_cast<const Half4*>(row);
      if constexpr (NOISE) logvar = *reinterpret_cast<const Half4*>(row + L);
    }
    float4 n = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (NOISE) n = *reinterpret_cast<const float4*>(noise + i * 4);
    const float ns[4] = {n.x, n.y, n.z, n.w};
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float mu = half_of(mean.w[j >> 1], j & 1);
      y[j] = NOISE ? mixdq_vae_latent(mu, half_of(logvar.w[j >> 1], j & 1), ns[j], sf) : mixdq_vae_latent_mode(mu, sf);
    }
    *reinterpret_cast<float4*>(z + i * 4) = make_float4(y[0], y[1], y[2], y[3]);
  }
}

int grid_for(int64_t items) {
  int64_t blocks = (items + 255) / 256;
  if (blocks > (int64_t)kNumCU * 8) blocks = (int64_t)kNumCU * 8;
  return (int)blocks;
}

}  // namespace
}  // namespace mixdq

using namespace mixdq;

extern "C" int mixdq_image_to_nhwc8_f16(const void* img, int dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw,
                                        void* out_f16, int B, int C, int H, int W, mixdq_stream_t stream_) {
  if (B < 0 || H < 0 || W < 0 || C < 1 || C > 8) return MIXDQ_ERR_INVALID_ARG;
  if (dtype != MIXDQ_IMAGE_U8 && dtype != MIXDQ_IMAGE_F16 && dtype != MIXDQ_IMAGE_F32) return MIXDQ_ERR_INVALID_ARG;
  const int64_t pixels = (int64_t)B * H * W;
  if (pixels == 0) return MIXDQ_OK;                 // (an empty tensor has no storage: before the pointer checks)
  if (!img || !out_f16) return MIXDQ_ERR_INVALID_ARG;
  const int elem = dtype == MIXDQ_IMAGE_U8 ? 1 : dtype == MIXDQ_IMAGE_F16 ? 2 : 4;
  if ((uintptr_t)out_f16 % 16 || (uintptr_t)img % elem) return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  Half8* out = (Half8*)out_f16;
  const int blocks = grid_for(pixels);
  if (dtype == MIXDQ_IMAGE_U8)
    image_to_nhwc8_kernel<uint8_t><<<blocks, 256, 0, stream>>>((const uint8_t*)img, sb, sc, sh, sw, out, pixels, C, H, W);
  else if (dtype == MIXDQ_IMAGE_F16)
    image_to_nhwc8_kernel<__half><<<blocks, 256, 0, stream>>>((const __half*)img, sb, sc, sh, sw, out, pixels, C, H, W);
  else
    image_to_nhwc8_kernel<float><<<blocks, 256, 0, stream>>>((const float*)img, sb, sc, sh, sw, out, pixels, C, H, W);
  return launch_status();
}

extern "C" int mixdq_vae_latent_sample(const void* moments_f16, const float* noise_or_null, float* z, int64_t pixels,
                                       int L, float scaling_factor, mixdq_stream_t stream_) {
  if (pixels < 0 || L < 1) return MIXDQ_ERR_INVALID_ARG;
  if (L % 4) return MIXDQ_ERR_ALIGNMENT;
  const int64_t groups = pixels * (L / 4);
  if (groups == 0) return MIXDQ_OK;                 // (an empty tensor has no storage: before the pointer checks)
  if (!moments_f16 || !z) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)moments_f16 % 16 || (uintptr_t)noise_or_null % 16 || (uintptr_t)z % 16) return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  const __half* m = (const __half*)moments_f16;
  const int blocks = grid_for(groups);
#define V_LAUNCH(NZ, L4) \
  vae_latent_kernel<NZ, L4><<<blocks, 256, 0, stream>>>(m, noise_or_null, z, groups, L, scaling_factor)
  if (noise_or_null) {
    if (L == 4) V_LAUNCH(true, true); else V_LAUNCH(true, false);
  } else {
    if (L == 4) V_LAUNCH(false, true); else V_LAUNCH(false, false);
  }
#undef V_LAUNCH
  return launch_status();
}
