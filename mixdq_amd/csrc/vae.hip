// The two ends of the VAE encoder for gfx950: the image ingest in front of conv_in and the posterior sample behind
// quant_conv.  No reference counterpart: the reference reaches the VAE only through diffusers' pipeline.
//
//   mixdq_image_to_nhwc8_f16   [B, C <= 8, H, W] uint8 / FP16 / FP32 at any element strides -> FP16 [B, H, W, 8],
//                              channels C..7 zero: the 8-channel form conv_in takes on the MFMA tiles (2C % 16 == 0)
//   mixdq_vae_latent_sample    FP16 moments [B, h, w, 2L] (+ FP32 noise [B, h, w, L]) -> FP32 z [B, h, w, L]
//
// and the two launches inpainting adds around the VAE:
//
//   mixdq_mask_to_latent       image-resolution mask [B, H, W] uint8 / FP16 / FP32 at any element strides -> FP32
//                              [B, H/8, W/8] of 0.0 / 1.0: pixel (8i, 8j) (NEAREST) or any pixel of the 8x8 block (ANY)
//   mixdq_composite_u8         out = mask ? to_uint8(decoded) : original, uint8 [B, H, W, 3]: the pixels outside the
//                              mask come back bit-identical (the VAE round trip does not reproduce an image)
//
// and the two the 9-channel inpainting checkpoints add (their UNet reads the mask and the blanked image's latents):
//
//   mixdq_image_to_nhwc8_f16_masked   the ingest with every pixel under the mask stored as +0.0 (mid-grey)
//   mixdq_inpaint_cond_f16            FP32 latent mask [B, h, w] + FP32 latents [B, h, w, L <= 7] -> FP16 [B, h, w, 8]
//                                     (mask | latents | zeros): the padded form SDXLUNet.cond_term takes
//
// and the one InstructPix2Pix adds (its 8-channel UNet reads the unscaled image latents, zero in the unconditional rows):
//
//   mixdq_ip2p_cond_f16               FP16 moments [B, h, w, 2L] -> FP16 [rows * B, h, w, 8], rows 1 or 3: f16(mean *
//                                     scale) | zeros in the first two row blocks, the third block all +0.0
//
// Arithmetic: include/mixdq_math.h (mixdq_pixel_to_unit, mixdq_vae_latent[_mode]), FP32 round-to-nearest, never
// contracted.  Both are HBM-bound and grid-stride, one pixel (one group of four latent channels) per lane per trip;
// every load of a trip is requested before the first value is used, and each lane writes one 16-byte store.
#include "common.h"
#include "../../include/mixdq_math.h"

namespace mixdq {
namespace {

struct alignas(8) Half4 { uint32_t w[2]; };

__device__ __forceinline__ float half_of(uint32_t word, int hi) {
  __half_raw hr;
  hr.x = (unsigned short)(hi ? (word >> 16) : (word & 0xffffu));
  return __half2float(__half(hr));
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

// ---- inpainting: the mask's binarisation (diffusers': uint8 u / 255 >= 0.5, floats v >= 0.5; NaN compares false)
__device__ __forceinline__ bool mask_set(uint8_t u) { return u >= 128; }
__device__ __forceinline__ bool mask_set(__half h) { return __half2float(h) >= 0.5f; }
__device__ __forceinline__ bool mask_set(float f) { return f >= 0.5f; }

// eight consecutive elements of one mask row in the widest loads their size allows (the launcher checked alignment)
__device__ __forceinline__ void load_row8(const uint8_t* p, uint8_t (&v)[8]) {
  const uint2 w = *reinterpret_cast<const uint2*>(p);
  memcpy(v, &w, 8);
}
__device__ __forceinline__ void load_row8(const __half* p, __half (&v)[8]) {
  const uint4 w = *reinterpret_cast<const uint4*>(p);
  memcpy(v, &w, 16);
}
__device__ __forceinline__ void load_row8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// One lane = one latent pixel.  ANY reads its 8x8 block: WIDE one row per (pair of) vector load(s), otherwise element
// by element at the caller's strides.
template <typename T, bool ANY, bool WIDE>
__global__ __launch_bounds__(256) void mask_to_latent_kernel(const T* __restrict__ mask, int64_t sb, int64_t sh,
                                                             int64_t sw, float* __restrict__ out, int64_t pixels, int h,
                                                             int w) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += stride) {
    const int64_t row = i / w;
    const int x = (int)(i - row * w);
    const int64_t b = row / h;
    const int y = (int)(row - b * h);
    const T* px = mask + (b * sb + (int64_t)(8 * y) * sh + (int64_t)(8 * x) * sw);
    bool set = false;
    if constexpr (!ANY) {
      set = mask_set(*px);
    } else if constexpr (WIDE) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        T v[8];
        load_row8(px + r * sh, v);
#pragma unroll
        for (int c = 0; c < 8; ++c) set |= mask_set(v[c]);
      }
    } else {
      for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) set |= mask_set(px[r * sh + c * sw]);
    }
    out[i] = set ? 1.0f : 0.0f;
  }
}

// The ingest with the masked pixels blanked: image_to_nhwc8_kernel's loads and arithmetic, plus the pixel's mask value;
// a set pixel stores sixteen zero bytes (+0.0 in every channel), whatever its source holds.
template <typename T, typename M>
__global__ __launch_bounds__(256) void image_to_nhwc8_masked_kernel(const T* __restrict__ img, int64_t sb, int64_t sc,
                                                                    int64_t sh, int64_t sw, const M* __restrict__ mask,
                                                                    int64_t mb, int64_t mh, int64_t mw,
                                                                    Half8* __restrict__ out, int64_t pixels, int C, int H,
                                                                    int W) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += stride) {
    const int64_t row = i / W;
    const int x = (int)(i - row * W);
    const int64_t b = row / H;
    const int y = (int)(row - b * H);
    const T* px = img + (b * sb + y * sh + x * sw);
    const M mv = mask[b * mb + y * mh + x * mw];
    T v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = c < C ? px[c * sc] : T(0);     // channels >= C are never read
    const bool set = mask_set(mv);
    uint32_t h[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) h[c] = (c < C && !set) ? half_bits(ingest_value(v[c])) : 0u;
    Half8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o.w[j] = h[2 * j] | (h[2 * j + 1] << 16);
    out[i] = o;
  }
}

// One lane = one latent pixel: its mask value and its L latent values, as FP16 in one 16-byte row (mask | z | zeros).
// L4: the pixel's four latents are one 16-byte load (the launcher checked alignment).
template <bool L4>
__global__ __launch_bounds__(256) void inpaint_cond_kernel(const float* __restrict__ mask_lat,
                                                           const float* __restrict__ zl, Half8* __restrict__ out,
                                                           int64_t pixels, int L) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += stride) {
    float v[8];
    v[0] = mask_lat[i];
    if constexpr (L4) {
      const float4 z = *reinterpret_cast<const float4*>(zl + i * 4);
      v[1] = z.x; v[2] = z.y; v[3] = z.z; v[4] = z.w;
      v[5] = v[6] = v[7] = 0.0f;
    } else {
      const float* z = zl + i * (int64_t)L;
#pragma unroll
      for (int c = 1; c < 8; ++c) v[c] = c <= L ? z[c - 1] : 0.0f;    // latents >= L are never read
    }
    uint32_t h[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) h[c] = c <= L ? half_bits(v[c]) : 0u;
    Half8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o.w[j] = h[2 * j] | (h[2 * j + 1] << 16);
    out[i] = o;
  }
}

// One lane = one latent pixel of one image: the L means of its moments, scaled, as FP16 in one 16-byte row (mean | zeros),
// stored to the first min(ROWS, 2) row blocks of `out`; the third block (ROWS == 3) gets sixteen zero bytes.  Blocks are
// `total` = B * pixels_per_image rows apart.  L4: the pixel's four means are one 8-byte load (the launcher checked
// alignment).
template <int ROWS, bool L4>
__global__ __launch_bounds__(256) void ip2p_cond_kernel(const __half* __restrict__ moments, Half8* __restrict__ out,
                                                        int64_t total, int L, float scale) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    uint32_t h[8];
    if constexpr (L4) {
      const Half4 m = *reinterpret_cast<const Half4*>(moments + i * 8);
#pragma unroll
      for (int c = 0; c < 8; ++c)
        h[c] = c < 4 ? half_bits(mixdq_vae_latent_mode(half_of(m.w[c >> 1], c & 1), scale)) : 0u;
    } else {
      const __half* m = moments + i * (2 * (int64_t)L);
#pragma unroll
      for (int c = 0; c < 8; ++c)                                    // the log-variances and channels >= L are never read
        h[c] = c < L ? half_bits(mixdq_vae_latent_mode(__half2float(m[c]), scale)) : 0u;
    }
    Half8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o.w[j] = h[2 * j] | (h[2 * j + 1] << 16);
    out[i] = o;
    if constexpr (ROWS == 3) {
      out[total + i] = o;
      out[2 * total + i] = Half8{{0u, 0u, 0u, 0u}};
    }
  }
}

// One lane = one pixel: three decoded FP16 values, the mask value, three original bytes, three bytes out.
template <typename T>
__global__ __launch_bounds__(256) void composite_u8_kernel(const __half* __restrict__ dec, int64_t db, int64_t dc,
                                                           int64_t dh, int64_t dw, const uint8_t* __restrict__ orig,
                                                           int64_t ob, int64_t oc, int64_t oh, int64_t ow,
                                                           const T* __restrict__ mask, int64_t mb, int64_t mh, int64_t mw,
                                                           uint8_t* __restrict__ out, int64_t pixels, int H, int W) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += stride) {
    const int64_t row = i / W;
    const int x = (int)(i - row * W);
    const int64_t b = row / H;
    const int y = (int)(row - b * H);
    const __half* d = dec + (b * db + y * dh + x * dw);
    const uint8_t* o = orig + (b * ob + y * oh + x * ow);
    const bool set = mask_set(mask[b * mb + y * mh + x * mw]);
    const __half d0 = d[0], d1 = d[dc], d2 = d[2 * dc];
    const uint8_t o0 = o[0], o1 = o[oc], o2 = o[2 * oc];
    uint8_t* q = out + i * 3;
    q[0] = set ? mixdq_to_uint8(__half2float(d0)) : o0;
    q[1] = set ? mixdq_to_uint8(__half2float(d1)) : o1;
    q[2] = set ? mixdq_to_uint8(__half2float(d2)) : o2;
  }
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
  const int blocks = grid_blocks(pixels);
  with_image_type(dtype, [&](auto t) {
    using T = decltype(t);
    image_to_nhwc8_kernel<T><<<blocks, 256, 0, stream>>>((const T*)img, sb, sc, sh, sw, out, pixels, C, H, W);
  });
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
  const int blocks = grid_blocks(groups);
  with_bool(noise_or_null != nullptr, [&](auto nz) {
    with_bool(L == 4, [&](auto l4) {
      vae_latent_kernel<decltype(nz)::value, decltype(l4)::value><<<blocks, 256, 0, stream>>>(
          m, noise_or_null, z, groups, L, scaling_factor);
    });
  });
  return launch_status();
}

namespace {
template <typename T>
void launch_mask_to_latent(const void* mask, int64_t sb, int64_t sh, int64_t sw, float* out, int64_t pixels, int h, int w,
                           int mode, hipStream_t stream) {
  const T* m = (const T*)mask;
  const int blocks = grid_blocks(pixels);
  // a row of 8 elements as one 8-byte (uint8) or 16-byte load(s): every row start must be aligned to that
  const int64_t align = sizeof(T) == 1 ? 8 : 16;
  const bool wide = sw == 1 && (uintptr_t)mask % align == 0 && (sh * (int64_t)sizeof(T)) % align == 0 &&
                    (sb * (int64_t)sizeof(T)) % align == 0;
  with_bool(mode != MIXDQ_MASK_NEAREST, [&](auto any) {
    with_bool(wide, [&](auto w8) {
      constexpr bool ANY = decltype(any)::value, WIDE = decltype(w8)::value;
      // (nearest reads one element per latent pixel: it has no wide form)
      mask_to_latent_kernel<T, ANY, ANY && WIDE><<<blocks, 256, 0, stream>>>(m, sb, sh, sw, out, pixels, h, w);
    });
  });
}
}  // namespace

extern "C" int mixdq_mask_to_latent(const void* mask, int dtype, int64_t sb, int64_t sh, int64_t sw, float* out, int B,
                                    int H, int W, int mode, mixdq_stream_t stream_) {
  const int elem = image_elem_size(dtype);
  if (B < 0 || H < 0 || W < 0 || H % 8 || W % 8 || !elem) return MIXDQ_ERR_INVALID_ARG;
  if (mode != MIXDQ_MASK_NEAREST && mode != MIXDQ_MASK_ANY) return MIXDQ_ERR_INVALID_ARG;
  if ((int64_t)B * H * W == 0) return MIXDQ_OK;     // (an empty tensor has no storage: before the pointer checks)
  if (!mask || !out) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)out % 4 || (uintptr_t)mask % elem) return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  const int h = H / 8, w = W / 8;
  const int64_t pixels = (int64_t)B * h * w;
  with_image_type(dtype, [&](auto t) {
    launch_mask_to_latent<decltype(t)>(mask, sb, sh, sw, out, pixels, h, w, mode, stream);
  });
  return launch_status();
}

extern "C" int mixdq_composite_u8(const void* decoded_f16, int64_t db, int64_t dc, int64_t dh, int64_t dw,
                                  const uint8_t* original, int64_t ob, int64_t oc, int64_t oh, int64_t ow,
                                  const void* mask, int mask_dtype, int64_t mb, int64_t mh, int64_t mw, uint8_t* out,
                                  int B, int H, int W, mixdq_stream_t stream_) {
  const int elem = image_elem_size(mask_dtype);
  if (B < 0 || H < 0 || W < 0 || !elem) return MIXDQ_ERR_INVALID_ARG;
  const int64_t pixels = (int64_t)B * H * W;
  if (pixels == 0) return MIXDQ_OK;                 // (an empty tensor has no storage: before the pointer checks)
  if (!decoded_f16 || !original || !mask || !out) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)decoded_f16 % 2 || (uintptr_t)mask % elem) return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  const __half* d = (const __half*)decoded_f16;
  const int blocks = grid_blocks(pixels);
  with_image_type(mask_dtype, [&](auto t) {
    using T = decltype(t);
    composite_u8_kernel<T><<<blocks, 256, 0, stream>>>(d, db, dc, dh, dw, original, ob, oc, oh, ow, (const T*)mask, mb,
                                                       mh, mw, out, pixels, H, W);
  });
  return launch_status();
}

namespace {
template <typename T>
void launch_ingest_masked(const void* img, int64_t sb, int64_t sc, int64_t sh, int64_t sw, const void* mask,
                          int mask_dtype, int64_t mb, int64_t mh, int64_t mw, Half8* out, int64_t pixels, int C, int H,
                          int W, hipStream_t stream) {
  const int blocks = grid_blocks(pixels);
  with_image_type(mask_dtype, [&](auto mt) {
    using M = decltype(mt);
    image_to_nhwc8_masked_kernel<T, M><<<blocks, 256, 0, stream>>>((const T*)img, sb, sc, sh, sw, (const M*)mask, mb,
                                                                   mh, mw, out, pixels, C, H, W);
  });
}
}  // namespace

extern "C" int mixdq_image_to_nhwc8_f16_masked(const void* img, int dtype, int64_t sb, int64_t sc, int64_t sh,
                                               int64_t sw, const void* mask, int mask_dtype, int64_t mb, int64_t mh,
                                               int64_t mw, void* out_f16, int B, int C, int H, int W,
                                               mixdq_stream_t stream_) {
  const int elem = image_elem_size(dtype), melem = image_elem_size(mask_dtype);
  if (B < 0 || H < 0 || W < 0 || C < 1 || C > 8 || !elem || !melem) return MIXDQ_ERR_INVALID_ARG;
  const int64_t pixels = (int64_t)B * H * W;
  if (pixels == 0) return MIXDQ_OK;                 // (an empty tensor has no storage: before the pointer checks)
  if (!img || !mask || !out_f16) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)out_f16 % 16 || (uintptr_t)img % elem || (uintptr_t)mask % melem) return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  Half8* out = (Half8*)out_f16;
  with_image_type(dtype, [&](auto t) {
    launch_ingest_masked<decltype(t)>(img, sb, sc, sh, sw, mask, mask_dtype, mb, mh, mw, out, pixels, C, H, W, stream);
  });
  return launch_status();
}

extern "C" int mixdq_inpaint_cond_f16(const float* mask_lat, const float* zl, void* out_f16, int64_t pixels, int L,
                                      mixdq_stream_t stream_) {
  if (pixels < 0 || L < 1 || L > 7) return MIXDQ_ERR_INVALID_ARG;
  if (pixels == 0) return MIXDQ_OK;                 // (an empty tensor has no storage: before the pointer checks)
  if (!mask_lat || !zl || !out_f16) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)out_f16 % 16 || (uintptr_t)mask_lat % 4 || (uintptr_t)zl % 4) return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  Half8* out = (Half8*)out_f16;
  const int blocks = grid_blocks(pixels);
  with_bool(L == 4 && (uintptr_t)zl % 16 == 0, [&](auto l4) {
    inpaint_cond_kernel<decltype(l4)::value><<<blocks, 256, 0, stream>>>(mask_lat, zl, out, pixels, L);
  });
  return launch_status();
}

extern "C" int mixdq_ip2p_cond_f16(const void* moments_f16, void* out_f16, int B, int64_t pixels_per_image, int L,
                                   int rows, float scale, mixdq_stream_t stream_) {
  if (B < 0 || pixels_per_image < 0 || L < 1 || L > 8 || (rows != 1 && rows != 3)) return MIXDQ_ERR_INVALID_ARG;
  const int64_t total = (int64_t)B * pixels_per_image;
  if (total == 0) return MIXDQ_OK;                  // (an empty tensor has no storage: before the pointer checks)
  if (!moments_f16 || !out_f16) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)out_f16 % 16 || (uintptr_t)moments_f16 % 2) return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  const __half* m = (const __half*)moments_f16;
  Half8* out = (Half8*)out_f16;
  const int blocks = grid_blocks(total);
  const bool l4 = L == 4 && (uintptr_t)moments_f16 % 8 == 0;
  with_constant<1, 3>(rows, [&](auto r) {
    with_bool(l4, [&](auto v) {
      ip2p_cond_kernel<decltype(r)::value, decltype(v)::value><<<blocks, 256, 0, stream>>>(m, out, total, L, scale);
    });
  });
  return launch_status();
}
