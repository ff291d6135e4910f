// Sampler step for gfx950: classifier-free guidance + the scheduler update + the UNet's next input, one launch,
// and the device-side step state (step index, the timestep the UNet reads) in a one-thread launch behind it.
// No reference counterpart: the reference reaches the sampling loop only through diffusers' pipeline call.
//
// Euler, Euler-ancestral, DDIM and LCM with an epsilon-predicting model are one affine map with per-step scalars:
//   e  = eps_u + g * (eps_c - eps_u)      (rows_per_image == 2; == 1: e = eps_u)
//   x' = (a*x + b*e) + c*n                (no noise pointer: a*x + b*e)
//   in = f16_rn(x' * s_next)              written to every UNet row of the image
// with (a, b, c, s_next) = coef[*step] -- arithmetic: include/mixdq_math.h, FP32 round-to-nearest, no contraction.
//
// HBM-bound and small (SDXL at 1024 px: 65 536 elements per image): elementwise over storage, 8 elements per lane
// per pass -- 16-byte accesses on the FP16 tensors, two on the FP32 ones -- and a scalar tail for n % 8 elements.
//
// mixdq_sampler_step_masked (inpainting) is the same step with one more map behind the update, in a sibling kernel:
//   k   = p*z + q*n0,   x'' = (1 - m)*k + m*x'     (p, q) = blend[*step], m = mask[i / channels]
// three more FP32 reads per element (z, n0 as 16-byte loads; the mask one value per latent pixel), x'' stored to x
// and in = f16_rn(x'' * s_next).  The four plain instantiations are untouched by it.
//
// mixdq_sampler_step_2m[_masked] (DPM-Solver++ 2M) is NOT one affine map of (x, eps, noise): a second-order step also
// reads the previous step's data prediction.  That one value per element is the only state a multistep solver adds; it
// lives in a caller-owned FP32 buffer `hist` that a third kernel (sampler_step_2m_kernel, below the two others, which
// it does not touch) reads and rewrites, with the index of the run's first step in a device int beside the step index.
//
// mixdq_sampler_step[_masked]_rng are the first two kernels in a third noise mode: n is not loaded but computed in
// registers -- Philox4x32-10 keyed by the image's seed, counter (element / 4, *step, stream 1), then Box-Muller
// (include/mixdq_math.h: mixdq_rng_*) -- so a stochastic schedule needs no [n_steps, ...] noise buffer and a captured
// graph serves every seed (the seeds are read from device memory).  mixdq_randn_f32 fills a buffer by the same rule
// (the start noise, the VAE posterior's), mixdq_rng_normals_from_bits is the words-to-normals map alone, for tests.
//
// The step index is read by every workgroup of the step launch and advanced by the launch BEHIND it on the same
// stream (sampler_advance_kernel, one thread): launches of one stream run in order, so no workgroup of the step
// can read the index after it moved, without any in-launch ticket, fence or counter to re-initialise.
#include "common.h"
#include "../../include/mixdq_math.h"

namespace mixdq {
namespace {

struct alignas(16) Half8 { uint32_t w[4]; };

__device__ __forceinline__ float half_at(const Half8& h, int j) {
  const uint32_t w = h.w[j >> 1];
  __half_raw hr;
  hr.x = (unsigned short)((j & 1) ? (w >> 16) : (w & 0xffffu));
  return __half2float(__half(hr));
}

__device__ __forceinline__ uint32_t half_bits(float v) {
  return (uint32_t)__half_raw(f32_to_f16_rn(v)).x;
}

// NOISE, the step kernels' noise mode: 0 none, 1 read from a buffer, 2 and 3 computed in registers (mixdq_rng_*,
// include/mixdq_math.h) from (seeds[image], element in the image, *step) on stream MIXDQ_RNG_STREAM_STEP.  An 8-element
// pass starting at storage element o: 2 (n_image % 8 == 0) -- it lies inside one image and is two whole Philox calls;
// 3 -- any n_image: one call per element, the image index carried along.  Roughly 300 vector operations per 8 elements
// in mode 2 against a 32-byte load in mode 1.
template <bool WHOLE>
__device__ __forceinline__ void rng_noise8(const uint64_t* __restrict__ seeds, int64_t n_image, int64_t o, uint32_t step,
                                           float ns[8]) {
  int64_t b = o / n_image;
  int64_t e = o - b * n_image;
  if (WHOLE) {
    const uint64_t seed = seeds[b];
    mixdq_rng_quad(seed, (uint64_t)e >> 2, step, MIXDQ_RNG_STREAM_STEP, ns);
    mixdq_rng_quad(seed, ((uint64_t)e >> 2) + 1, step, MIXDQ_RNG_STREAM_STEP, ns + 4);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {                  // o + j < n and n % n_image == 0: b stays below n / n_image
      ns[j] = mixdq_rng_normal_at(seeds[b], (uint64_t)e, step, MIXDQ_RNG_STREAM_STEP);
      if (++e == n_image) { e = 0; ++b; }
    }
  }
}

template <int NOISE>
__device__ __forceinline__ float tail_noise(const float* __restrict__ nz, const uint64_t* __restrict__ seeds,
                                            int64_t n_image, int64_t t, uint32_t step) {
  if (NOISE == 0) return 0.0f;
  if (NOISE == 1) return nz[t];
  const int64_t b = t / n_image;
  return mixdq_rng_normal_at(seeds[b], (uint64_t)(t - b * n_image), step, MIXDQ_RNG_STREAM_STEP);
}

// mixdq_randn_f32: one Philox call -- four normals -- per lane per pass, grid-stride over the B * ceil(n_image / 4) calls.
// VEC (n_image % 4 == 0): every call's four elements are one aligned 16-byte store; otherwise the last call of an image
// is partly used and the stores are scalar.
template <bool VEC>
__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, int64_t n_image, int64_t quads_per_image,
                                                    int64_t total_quads, const uint64_t* __restrict__ seeds,
                                                    uint32_t rstream, uint32_t step) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total_quads; q += stride) {
    const int64_t b = q / quads_per_image;         // q < B * quads_per_image: b < B
    const int64_t qi = q - b * quads_per_image;
    float z[4];
    mixdq_rng_quad(seeds[b], (uint64_t)qi, step, rstream, z);
    float* p = out + b * n_image + 4 * qi;
    if (VEC) {
      *reinterpret_cast<float4*>(p) = make_float4(z[0], z[1], z[2], z[3]);
    } else {
      const int64_t left = n_image - 4 * qi;       // >= 1
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < left) p[j] = z[j];
    }
  }
}

__global__ __launch_bounds__(256) void normals_from_bits_kernel(const uint32_t* __restrict__ r, float* __restrict__ z,
                                                                int64_t n_quads) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_quads; q += stride) {
    const uint4 w = *reinterpret_cast<const uint4*>(r + 4 * q);
    const uint32_t rr[4] = {w.x, w.y, w.z, w.w};
    float zz[4];
    mixdq_rng_normals4(rr, zz);
    *reinterpret_cast<float4*>(z + 4 * q) = make_float4(zz[0], zz[1], zz[2], zz[3]);
  }
}

template <int ROWS, int NOISE>
__device__ __forceinline__ float step_one(float x, float eu, float ec, float n, float g, float a, float b, float c) {
  const float e = ROWS == 2 ? mixdq_sampler_guided_eps(eu, ec, g) : eu;
  return NOISE ? mixdq_sampler_update_noise(x, e, n, a, b, c) : mixdq_sampler_update(x, e, a, b);
}

template <int ROWS, int NOISE>
__global__ __launch_bounds__(256) void sampler_step_kernel(float* __restrict__ x, const __half* __restrict__ eps,
                                                           __half* __restrict__ in, const float* __restrict__ noise,
                                                           int64_t noise_stride, const float* __restrict__ coef,
                                                           const int* __restrict__ step_p, int n_steps, float g,
                                                           int64_t n, int64_t row_stride,
                                                           const uint64_t* __restrict__ seeds, int64_t n_image) {
  const int step = *step_p;
  if (step < 0 || step >= n_steps) return;        // replayed past the table: nothing is read or written
  const float4 k = *reinterpret_cast<const float4*>(coef + 4 * (int64_t)step);
  const float a = k.x, b = k.y, c = k.z, s_next = k.w;
  const float* nz = NOISE == 1 ? noise + (int64_t)step * noise_stride : nullptr;
  const int64_t nvec = n >> 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const int64_t o = i << 3;
    const float4 x0 = *reinterpret_cast<const float4*>(x + o), x1 = *reinterpret_cast<const float4*>(x + o + 4);
    const Half8 eu = *reinterpret_cast<const Half8*>(eps + o);
    Half8 ec = eu;
    if (ROWS == 2) ec = *reinterpret_cast<const Half8*>(eps + row_stride + o);
    float4 n0 = x0, n1 = x1;
    if (NOISE == 1) {
      n0 = *reinterpret_cast<const float4*>(nz + o);
      n1 = *reinterpret_cast<const float4*>(nz + o + 4);
    }
    const float xs[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    float ns[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
    if (NOISE >= 2) rng_noise8<NOISE == 2>(seeds, n_image, o, (uint32_t)step, ns);
    float y[8];
    Half8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = step_one<ROWS, NOISE>(xs[j], half_at(eu, j), half_at(ec, j), ns[j], g, a, b, c);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      out.w[j] = half_bits(mixdq_sampler_scaled_input(y[2 * j], s_next)) |
                 (half_bits(mixdq_sampler_scaled_input(y[2 * j + 1], s_next)) << 16);
    *reinterpret_cast<float4*>(x + o) = make_float4(y[0], y[1], y[2], y[3]);
    *reinterpret_cast<float4*>(x + o + 4) = make_float4(y[4], y[5], y[6], y[7]);
    *reinterpret_cast<Half8*>(in + o) = out;
    if (ROWS == 2) *reinterpret_cast<Half8*>(in + row_stride + o) = out;
  }
  // tail (n % 8 elements), by the first threads of block 0
  const int64_t t = (nvec << 3) + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    const float eu = __half2float(eps[t]);
    const float ec = ROWS == 2 ? __half2float(eps[row_stride + t]) : eu;
    const float y = step_one<ROWS, NOISE>(x[t], eu, ec, tail_noise<NOISE>(nz, seeds, n_image, t, (uint32_t)step), g, a, b, c);
    const __half h = f32_to_f16_rn(mixdq_sampler_scaled_input(y, s_next));
    x[t] = y;
    in[t] = h;
    if (ROWS == 2) in[row_stride + t] = h;
  }
}

// The masked step: sampler_step_kernel's body, then mixdq_sampler_blend.  Element i of the (channels-last) storage
// belongs to mask entry i / channels.  C4: channels == 4, an 8-element pass covers exactly two latent pixels; otherwise
// the quotient and remainder of the pass's first element are divided out once and carried along.
template <int ROWS, int NOISE, bool C4>
__global__ __launch_bounds__(256) void sampler_step_masked_kernel(
    float* __restrict__ x, const __half* __restrict__ eps, __half* __restrict__ in, const float* __restrict__ noise,
    int64_t noise_stride, const float* __restrict__ coef, const int* __restrict__ step_p, int n_steps, float g, int64_t n,
    int64_t row_stride, const float* __restrict__ z, const float* __restrict__ noise0, const float* __restrict__ mask,
    int channels, const float* __restrict__ blend, const uint64_t* __restrict__ seeds, int64_t n_image) {
  const int step = *step_p;
  if (step < 0 || step >= n_steps) return;        // replayed past the table: nothing is read or written
  const float4 k = *reinterpret_cast<const float4*>(coef + 4 * (int64_t)step);
  const float a = k.x, b = k.y, c = k.z, s_next = k.w;
  const float2 pq = *reinterpret_cast<const float2*>(blend + 2 * (int64_t)step);
  const float* nz = NOISE == 1 ? noise + (int64_t)step * noise_stride : nullptr;
  const int64_t nvec = n >> 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const int64_t o = i << 3;
    const float4 x0 = *reinterpret_cast<const float4*>(x + o), x1 = *reinterpret_cast<const float4*>(x + o + 4);
    const float4 z0 = *reinterpret_cast<const float4*>(z + o), z1 = *reinterpret_cast<const float4*>(z + o + 4);
    const float4 i0 = *reinterpret_cast<const float4*>(noise0 + o), i1 = *reinterpret_cast<const float4*>(noise0 + o + 4);
    const Half8 eu = *reinterpret_cast<const Half8*>(eps + o);
    Half8 ec = eu;
    if (ROWS == 2) ec = *reinterpret_cast<const Half8*>(eps + row_stride + o);
    float4 n0 = x0, n1 = x1;
    if (NOISE == 1) {
      n0 = *reinterpret_cast<const float4*>(nz + o);
      n1 = *reinterpret_cast<const float4*>(nz + o + 4);
    }
    float ms[8];
    if (C4) {
      const float m0 = mask[2 * i], m1 = mask[2 * i + 1];
#pragma unroll
      for (int j = 0; j < 8; ++j) ms[j] = j < 4 ? m0 : m1;
    } else {
      int64_t q = o / channels;                    // o + j < n and n % channels == 0: q stays below n / channels
      int r = (int)(o - q * channels);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ms[j] = mask[q];
        if (++r == channels) { r = 0; ++q; }
      }
    }
    const float xs[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    float ns[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
    if (NOISE >= 2) rng_noise8<NOISE == 2>(seeds, n_image, o, (uint32_t)step, ns);
    const float zs[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
    const float is[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
    float y[8];
    Half8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      y[j] = mixdq_sampler_blend(step_one<ROWS, NOISE>(xs[j], half_at(eu, j), half_at(ec, j), ns[j], g, a, b, c), zs[j],
                                 is[j], ms[j], pq.x, pq.y);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      out.w[j] = half_bits(mixdq_sampler_scaled_input(y[2 * j], s_next)) |
                 (half_bits(mixdq_sampler_scaled_input(y[2 * j + 1], s_next)) << 16);
    *reinterpret_cast<float4*>(x + o) = make_float4(y[0], y[1], y[2], y[3]);
    *reinterpret_cast<float4*>(x + o + 4) = make_float4(y[4], y[5], y[6], y[7]);
    *reinterpret_cast<Half8*>(in + o) = out;
    if (ROWS == 2) *reinterpret_cast<Half8*>(in + row_stride + o) = out;
  }
  // tail (n % 8 elements), by the first threads of block 0
  const int64_t t = (nvec << 3) + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    const float eu = __half2float(eps[t]);
    const float ec = ROWS == 2 ? __half2float(eps[row_stride + t]) : eu;
    const float y = mixdq_sampler_blend(step_one<ROWS, NOISE>(x[t], eu, ec, tail_noise<NOISE>(nz, seeds, n_image, t, (uint32_t)step), g, a, b, c), z[t],
                                        noise0[t], mask[t / channels], pq.x, pq.y);
    const __half h = f32_to_f16_rn(mixdq_sampler_scaled_input(y, s_next));
    x[t] = y;
    in[t] = h;
    if (ROWS == 2) in[row_stride + t] = h;
  }
}

// The multistep step (DPM-Solver++ 2M, mixdq_sampler_step_2m[_masked]): the data prediction x0 = u*x + v*e, then a
// first- or second-order update of x from x0 and the PREVIOUS step's x0, which lives in `hist` (FP32, x's layout) and is
// replaced by this step's on every launch.  (u, v, A, B1, B2, D2, s_next, 0) = coef8[*step].  Which order a step takes
// depends on the table and on two device scalars only -- the first executed step of a run (*step == *first) and a row
// with D2 == 0 are first-order -- so the choice is uniform over the launch and `hist` is not read at all on a
// first-order step: it may hold anything there.  One more FP32 read (second-order steps) and write per element than the
// plain step; these kinds add no noise.  MASKED: 0 none, 1 the blend with channels == 4, 2 with any channel count;
// the blend touches x and the UNet input, never `hist`.
template <int ROWS>
__device__ __forceinline__ float step_2m_one(float x, float eu, float ec, float h, float g, float u, float v, float A,
                                             float B, float D, bool second, float* x0_out) {
  const float e = ROWS == 2 ? mixdq_sampler_guided_eps(eu, ec, g) : eu;
  const float x0 = mixdq_sampler_x0(x, e, u, v);
  *x0_out = x0;
  return second ? mixdq_sampler_update_2m(x, x0, h, A, B, D) : mixdq_sampler_update(x, x0, A, B);
}

template <int ROWS, int MASKED>
__global__ __launch_bounds__(256) void sampler_step_2m_kernel(
    float* __restrict__ x, const __half* __restrict__ eps, __half* __restrict__ in, float* __restrict__ hist,
    const float* __restrict__ coef8, const int* __restrict__ step_p, const int* __restrict__ first_p, int n_steps, float g,
    int64_t n, int64_t row_stride, const float* __restrict__ z, const float* __restrict__ noise0,
    const float* __restrict__ mask, int channels, const float* __restrict__ blend) {
  const int step = *step_p;
  if (step < 0 || step >= n_steps) return;        // replayed past the table: nothing is read or written
  const float4 k0 = *reinterpret_cast<const float4*>(coef8 + 8 * (int64_t)step);
  const float4 k1 = *reinterpret_cast<const float4*>(coef8 + 8 * (int64_t)step + 4);
  const float u = k0.x, v = k0.y, A = k0.z, D = k1.y, s_next = k1.z;
  const bool second = step > *first_p && D != 0.0f;
  const float B = second ? k1.x : k0.w;
  float2 pq = make_float2(1.0f, 0.0f);
  if (MASKED) pq = *reinterpret_cast<const float2*>(blend + 2 * (int64_t)step);
  const int64_t nvec = n >> 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const int64_t o = i << 3;
    const float4 x0 = *reinterpret_cast<const float4*>(x + o), x1 = *reinterpret_cast<const float4*>(x + o + 4);
    const Half8 eu = *reinterpret_cast<const Half8*>(eps + o);
    Half8 ec = eu;
    if (ROWS == 2) ec = *reinterpret_cast<const Half8*>(eps + row_stride + o);
    float4 h0 = x0, h1 = x1;
    if (second) {
      h0 = *reinterpret_cast<const float4*>(hist + o);
      h1 = *reinterpret_cast<const float4*>(hist + o + 4);
    }
    float4 z0 = x0, z1 = x1, i0 = x0, i1 = x1;
    float ms[8];
    if (MASKED) {
      z0 = *reinterpret_cast<const float4*>(z + o);
      z1 = *reinterpret_cast<const float4*>(z + o + 4);
      i0 = *reinterpret_cast<const float4*>(noise0 + o);
      i1 = *reinterpret_cast<const float4*>(noise0 + o + 4);
      if (MASKED == 1) {
        const float m0 = mask[2 * i], m1 = mask[2 * i + 1];
#pragma unroll
        for (int j = 0; j < 8; ++j) ms[j] = j < 4 ? m0 : m1;
      } else {
        int64_t q = o / channels;                  // o + j < n and n % channels == 0: q stays below n / channels
        int r = (int)(o - q * channels);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          ms[j] = mask[q];
          if (++r == channels) { r = 0; ++q; }
        }
      }
    }
    const float xs[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    const float hs[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
    const float zs[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
    const float is[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
    float y[8], p0[8];
    Half8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      y[j] = step_2m_one<ROWS>(xs[j], half_at(eu, j), half_at(ec, j), hs[j], g, u, v, A, B, D, second, &p0[j]);
      if (MASKED) y[j] = mixdq_sampler_blend(y[j], zs[j], is[j], ms[j], pq.x, pq.y);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      out.w[j] = half_bits(mixdq_sampler_scaled_input(y[2 * j], s_next)) |
                 (half_bits(mixdq_sampler_scaled_input(y[2 * j + 1], s_next)) << 16);
    *reinterpret_cast<float4*>(hist + o) = make_float4(p0[0], p0[1], p0[2], p0[3]);
    *reinterpret_cast<float4*>(hist + o + 4) = make_float4(p0[4], p0[5], p0[6], p0[7]);
    *reinterpret_cast<float4*>(x + o) = make_float4(y[0], y[1], y[2], y[3]);
    *reinterpret_cast<float4*>(x + o + 4) = make_float4(y[4], y[5], y[6], y[7]);
    *reinterpret_cast<Half8*>(in + o) = out;
    if (ROWS == 2) *reinterpret_cast<Half8*>(in + row_stride + o) = out;
  }
  // tail (n % 8 elements), by the first threads of block 0
  const int64_t t = (nvec << 3) + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    const float eu = __half2float(eps[t]);
    const float ec = ROWS == 2 ? __half2float(eps[row_stride + t]) : eu;
    const float xt = x[t];
    float p0;
    float y = step_2m_one<ROWS>(xt, eu, ec, second ? hist[t] : xt, g, u, v, A, B, D, second, &p0);
    if (MASKED) y = mixdq_sampler_blend(y, z[t], noise0[t], mask[t / channels], pq.x, pq.y);
    const __half h = f32_to_f16_rn(mixdq_sampler_scaled_input(y, s_next));
    hist[t] = p0;
    x[t] = y;
    in[t] = h;
    if (ROWS == 2) in[row_stride + t] = h;
  }
}

// Behind the step on the same stream: the timestep of the NEXT UNet forward, and the index moves on.
__global__ void sampler_advance_kernel(const float* __restrict__ t_table, int n_steps, int* step_p, float* timestep) {
  const int step = *step_p;
  if (step < 0 || step >= n_steps) return;
  *timestep = t_table[step + 1];
  *step_p = step + 1;
}

// The argument checks of both entry points, in mixdq_sampler_step's order.
int check_step_args(const float* x, const void* eps_f16, const void* in_f16, const float* noise_or_null,
                    int64_t noise_stride, const float* coef, const float* t_table, int n_steps, const int* step,
                    const float* timestep, int64_t n, int rows_per_image, int64_t row_stride) {
  if (!x || !eps_f16 || !in_f16 || !coef || !t_table || !step || !timestep) return MIXDQ_ERR_INVALID_ARG;
  if (n < 0 || n_steps < 1 || (rows_per_image != 1 && rows_per_image != 2)) return MIXDQ_ERR_INVALID_ARG;
  if (rows_per_image == 2 && row_stride < n) return MIXDQ_ERR_INVALID_ARG;      // the two row blocks would overlap
  if (noise_or_null && noise_stride < n) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)x % 16 || (uintptr_t)eps_f16 % 16 || (uintptr_t)in_f16 % 16 || (uintptr_t)coef % 16 ||
      (uintptr_t)noise_or_null % 16 || (uintptr_t)t_table % 4 || (uintptr_t)step % 4 || (uintptr_t)timestep % 4)
    return MIXDQ_ERR_ALIGNMENT;
  if ((rows_per_image == 2 && row_stride % 8) || (noise_or_null && noise_stride % 4)) return MIXDQ_ERR_ALIGNMENT;
  return MIXDQ_OK;
}

int step_blocks(int64_t n) {
  int64_t blocks = ((n >> 3) + 255) / 256;
  if (blocks > (int64_t)kNumCU * 8) blocks = (int64_t)kNumCU * 8;
  return blocks < 1 ? 1 : (int)blocks;
}

}  // namespace
}  // namespace mixdq

using namespace mixdq;

extern "C" int mixdq_sampler_step(float* x, const void* eps_f16, void* in_f16, const float* noise_or_null,
                                  int64_t noise_stride, const float* coef, const float* t_table, int n_steps,
                                  int* step, float* timestep, float guidance, int64_t n, int rows_per_image,
                                  int64_t row_stride, mixdq_stream_t stream_) {
  const int bad = check_step_args(x, eps_f16, in_f16, noise_or_null, noise_stride, coef, t_table, n_steps, step, timestep,
                                  n, rows_per_image, row_stride);
  if (bad != MIXDQ_OK) return bad;
  hipStream_t stream = (hipStream_t)stream_;
  if (n > 0) {
    const int blocks = step_blocks(n);
    const __half* eps = (const __half*)eps_f16;
    __half* in = (__half*)in_f16;
#define S_LAUNCH(R, NZ)                                                                               \
  sampler_step_kernel<R, NZ><<<blocks, 256, 0, stream>>>(x, eps, in, noise_or_null, noise_stride, coef, step, \
                                                         n_steps, guidance, n, row_stride, nullptr, 0)
    if (rows_per_image == 2) {
      if (noise_or_null) S_LAUNCH(2, 1); else S_LAUNCH(2, 0);
    } else {
      if (noise_or_null) S_LAUNCH(1, 1); else S_LAUNCH(1, 0);
    }
#undef S_LAUNCH
    if (hipGetLastError() != hipSuccess) return MIXDQ_ERR_LAUNCH;
  }
  sampler_advance_kernel<<<1, 1, 0, stream>>>(t_table, n_steps, step, timestep);
  return launch_status();
}

extern "C" int mixdq_sampler_step_masked(float* x, const void* eps_f16, void* in_f16, const float* noise_or_null,
                                         int64_t noise_stride, const float* coef, const float* t_table, int n_steps,
                                         int* step, float* timestep, float guidance, int64_t n, int rows_per_image,
                                         int64_t row_stride, const float* z, const float* noise0, const float* mask,
                                         int channels, const float* blend, mixdq_stream_t stream_) {
  const int bad = check_step_args(x, eps_f16, in_f16, noise_or_null, noise_stride, coef, t_table, n_steps, step, timestep,
                                  n, rows_per_image, row_stride);
  if (bad != MIXDQ_OK) return bad;
  if (!z || !noise0 || !mask || !blend || channels < 1 || n % channels) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)z % 16 || (uintptr_t)noise0 % 16 || (uintptr_t)mask % 4 || (uintptr_t)blend % 8)
    return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  if (n > 0) {
    const int blocks = step_blocks(n);
    const __half* eps = (const __half*)eps_f16;
    __half* in = (__half*)in_f16;
#define M_LAUNCH(R, NZ, C4)                                                                                          \
  sampler_step_masked_kernel<R, NZ, C4><<<blocks, 256, 0, stream>>>(x, eps, in, noise_or_null, noise_stride, coef, step, \
                                                                    n_steps, guidance, n, row_stride, z, noise0, mask,   \
                                                                    channels, blend, nullptr, 0)
#define M_LAUNCH_C(R, NZ) \
  do { if (channels == 4) M_LAUNCH(R, NZ, true); else M_LAUNCH(R, NZ, false); } while (0)
    if (rows_per_image == 2) {
      if (noise_or_null) M_LAUNCH_C(2, 1); else M_LAUNCH_C(2, 0);
    } else {
      if (noise_or_null) M_LAUNCH_C(1, 1); else M_LAUNCH_C(1, 0);
    }
#undef M_LAUNCH_C
#undef M_LAUNCH
    if (hipGetLastError() != hipSuccess) return MIXDQ_ERR_LAUNCH;
  }
  sampler_advance_kernel<<<1, 1, 0, stream>>>(t_table, n_steps, step, timestep);
  return launch_status();
}

// ---- noise made on the device ------------------------------------------------------------------------------------------
namespace mixdq {
namespace {

int quad_blocks(int64_t quads) {
  int64_t blocks = (quads + 255) / 256;
  if (blocks > (int64_t)kNumCU * 8) blocks = (int64_t)kNumCU * 8;
  return blocks < 1 ? 1 : (int)blocks;
}

// What the two _rng entry points check beyond check_step_args.
int check_rng_args(const uint64_t* seeds, int64_t n_image, int64_t n) {
  if (!seeds || n_image < 1 || n % n_image) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)seeds % 8) return MIXDQ_ERR_ALIGNMENT;
  return MIXDQ_OK;
}

}  // namespace
}  // namespace mixdq

extern "C" int mixdq_randn_f32(float* out, int B, int64_t n_image, const uint64_t* seeds_device, uint32_t rstream,
                               uint32_t step, mixdq_stream_t stream_) {
  if (!out || !seeds_device || B < 0 || n_image < 1) return MIXDQ_ERR_INVALID_ARG;
  const bool vec = n_image % 4 == 0;
  if ((uintptr_t)out % (vec ? 16 : 4) || (uintptr_t)seeds_device % 8) return MIXDQ_ERR_ALIGNMENT;
  if (B == 0) return MIXDQ_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t qpi = (n_image + 3) / 4, total = qpi * B;
  const int blocks = quad_blocks(total);
  if (vec) randn_kernel<true><<<blocks, 256, 0, stream>>>(out, n_image, qpi, total, seeds_device, rstream, step);
  else randn_kernel<false><<<blocks, 256, 0, stream>>>(out, n_image, qpi, total, seeds_device, rstream, step);
  return launch_status();
}

extern "C" int mixdq_rng_normals_from_bits(const uint32_t* r, float* z, int64_t n_quads, mixdq_stream_t stream_) {
  if (!r || !z || n_quads < 0) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)r % 16 || (uintptr_t)z % 16) return MIXDQ_ERR_ALIGNMENT;
  if (n_quads == 0) return MIXDQ_OK;
  normals_from_bits_kernel<<<quad_blocks(n_quads), 256, 0, (hipStream_t)stream_>>>(r, z, n_quads);
  return launch_status();
}

extern "C" int mixdq_sampler_step_rng(float* x, const void* eps_f16, void* in_f16, const uint64_t* seeds,
                                      int64_t n_image, const float* coef, const float* t_table, int n_steps, int* step,
                                      float* timestep, float guidance, int64_t n, int rows_per_image, int64_t row_stride,
                                      mixdq_stream_t stream_) {
  int bad = check_step_args(x, eps_f16, in_f16, nullptr, 0, coef, t_table, n_steps, step, timestep, n, rows_per_image,
                            row_stride);
  if (bad == MIXDQ_OK) bad = check_rng_args(seeds, n_image, n);
  if (bad != MIXDQ_OK) return bad;
  hipStream_t stream = (hipStream_t)stream_;
  if (n > 0) {
    const int blocks = step_blocks(n);
    const __half* eps = (const __half*)eps_f16;
    __half* in = (__half*)in_f16;
#define R_LAUNCH(R, NZ)                                                                                             \
  sampler_step_kernel<R, NZ><<<blocks, 256, 0, stream>>>(x, eps, in, nullptr, 0, coef, step, n_steps, guidance, n, \
                                                         row_stride, seeds, n_image)
    if (rows_per_image == 2) {
      if (n_image % 8 == 0) R_LAUNCH(2, 2); else R_LAUNCH(2, 3);
    } else {
      if (n_image % 8 == 0) R_LAUNCH(1, 2); else R_LAUNCH(1, 3);
    }
#undef R_LAUNCH
    if (hipGetLastError() != hipSuccess) return MIXDQ_ERR_LAUNCH;
  }
  sampler_advance_kernel<<<1, 1, 0, stream>>>(t_table, n_steps, step, timestep);
  return launch_status();
}

extern "C" int mixdq_sampler_step_masked_rng(float* x, const void* eps_f16, void* in_f16, const uint64_t* seeds,
                                             int64_t n_image, const float* coef, const float* t_table, int n_steps,
                                             int* step, float* timestep, float guidance, int64_t n, int rows_per_image,
                                             int64_t row_stride, const float* z, const float* noise0, const float* mask,
                                             int channels, const float* blend, mixdq_stream_t stream_) {
  int bad = check_step_args(x, eps_f16, in_f16, nullptr, 0, coef, t_table, n_steps, step, timestep, n, rows_per_image,
                            row_stride);
  if (bad == MIXDQ_OK) bad = check_rng_args(seeds, n_image, n);
  if (bad != MIXDQ_OK) return bad;
  if (!z || !noise0 || !mask || !blend || channels < 1 || n % channels) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)z % 16 || (uintptr_t)noise0 % 16 || (uintptr_t)mask % 4 || (uintptr_t)blend % 8)
    return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  if (n > 0) {
    const int blocks = step_blocks(n);
    const __half* eps = (const __half*)eps_f16;
    __half* in = (__half*)in_f16;
#define MR_LAUNCH(R, NZ, C4)                                                                                          \
  sampler_step_masked_kernel<R, NZ, C4><<<blocks, 256, 0, stream>>>(x, eps, in, nullptr, 0, coef, step, n_steps,      \
                                                                    guidance, n, row_stride, z, noise0, mask, channels, \
                                                                    blend, seeds, n_image)
#define MR_LAUNCH_C(R, NZ) \
  do { if (channels == 4) MR_LAUNCH(R, NZ, true); else MR_LAUNCH(R, NZ, false); } while (0)
    if (rows_per_image == 2) {
      if (n_image % 8 == 0) MR_LAUNCH_C(2, 2); else MR_LAUNCH_C(2, 3);
    } else {
      if (n_image % 8 == 0) MR_LAUNCH_C(1, 2); else MR_LAUNCH_C(1, 3);
    }
#undef MR_LAUNCH_C
#undef MR_LAUNCH
    if (hipGetLastError() != hipSuccess) return MIXDQ_ERR_LAUNCH;
  }
  sampler_advance_kernel<<<1, 1, 0, stream>>>(t_table, n_steps, step, timestep);
  return launch_status();
}

namespace mixdq {
namespace {

// What the two multistep entry points check beyond check_step_args (which sees coef8 as its table).
int check_2m_args(const float* x, const float* hist, const float* coef8, const int* first, int64_t n) {
  if (!hist || !coef8 || !first) return MIXDQ_ERR_INVALID_ARG;
  if (hist < x + n && x < hist + n) return MIXDQ_ERR_INVALID_ARG;                // the history is a buffer of its own
  if ((uintptr_t)hist % 16 || (uintptr_t)coef8 % 16 || (uintptr_t)first % 4) return MIXDQ_ERR_ALIGNMENT;
  return MIXDQ_OK;
}

}  // namespace
}  // namespace mixdq

extern "C" int mixdq_sampler_step_2m(float* x, const void* eps_f16, void* in_f16, float* hist, const float* coef8,
                                     const float* t_table, int n_steps, int* step, const int* first, float* timestep,
                                     float guidance, int64_t n, int rows_per_image, int64_t row_stride,
                                     mixdq_stream_t stream_) {
  int bad = check_step_args(x, eps_f16, in_f16, nullptr, 0, coef8, t_table, n_steps, step, timestep, n, rows_per_image,
                            row_stride);
  if (bad == MIXDQ_OK) bad = check_2m_args(x, hist, coef8, first, n);
  if (bad != MIXDQ_OK) return bad;
  hipStream_t stream = (hipStream_t)stream_;
  if (n > 0) {
    const int blocks = step_blocks(n);
    const __half* eps = (const __half*)eps_f16;
    __half* in = (__half*)in_f16;
#define S2_LAUNCH(R)                                                                                                  \
  sampler_step_2m_kernel<R, 0><<<blocks, 256, 0, stream>>>(x, eps, in, hist, coef8, step, first, n_steps, guidance, n, \
                                                           row_stride, nullptr, nullptr, nullptr, 1, nullptr)
    if (rows_per_image == 2) S2_LAUNCH(2); else S2_LAUNCH(1);
#undef S2_LAUNCH
    if (hipGetLastError() != hipSuccess) return MIXDQ_ERR_LAUNCH;
  }
  sampler_advance_kernel<<<1, 1, 0, stream>>>(t_table, n_steps, step, timestep);
  return launch_status();
}

extern "C" int mixdq_sampler_step_2m_masked(float* x, const void* eps_f16, void* in_f16, float* hist, const float* coef8,
                                            const float* t_table, int n_steps, int* step, const int* first,
                                            float* timestep, float guidance, int64_t n, int rows_per_image,
                                            int64_t row_stride, const float* z, const float* noise0, const float* mask,
                                            int channels, const float* blend, mixdq_stream_t stream_) {
  int bad = check_step_args(x, eps_f16, in_f16, nullptr, 0, coef8, t_table, n_steps, step, timestep, n, rows_per_image,
                            row_stride);
  if (bad == MIXDQ_OK) bad = check_2m_args(x, hist, coef8, first, n);
  if (bad != MIXDQ_OK) return bad;
  if (!z || !noise0 || !mask || !blend || channels < 1 || n % channels) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)z % 16 || (uintptr_t)noise0 % 16 || (uintptr_t)mask % 4 || (uintptr_t)blend % 8)
    return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  if (n > 0) {
    const int blocks = step_blocks(n);
    const __half* eps = (const __half*)eps_f16;
    __half* in = (__half*)in_f16;
#define M2_LAUNCH(R, M)                                                                                               \
  sampler_step_2m_kernel<R, M><<<blocks, 256, 0, stream>>>(x, eps, in, hist, coef8, step, first, n_steps, guidance, n, \
                                                           row_stride, z, noise0, mask, channels, blend)
    if (rows_per_image == 2) {
      if (channels == 4) M2_LAUNCH(2, 1); else M2_LAUNCH(2, 2);
    } else {
      if (channels == 4) M2_LAUNCH(1, 1); else M2_LAUNCH(1, 2);
    }
#undef M2_LAUNCH
    if (hipGetLastError() != hipSuccess) return MIXDQ_ERR_LAUNCH;
  }
  sampler_advance_kernel<<<1, 1, 0, stream>>>(t_table, n_steps, step, timestep);
  return launch_status();
}
