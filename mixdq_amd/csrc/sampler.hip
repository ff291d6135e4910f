// Sampler step for gfx950: classifier-free guidance + the scheduler update + the UNet's next input, one launch,
// and the device-side step state (step index, the timestep the UNet reads) in a one-thread launch behind it.
// No reference counterpart: the reference reaches the sampling loop only through diffusers' pipeline call.
//
// Every step is ONE kernel template, sampler_step_kernel<ROWS, ORDER, NOISE, MASK>: its own are the grid-stride loop
// and the tail; the body is sampler_step.h's, shared with the rescaled step (sampler_rescale.hip), built from
// include/mixdq_math.h -- FP32 round-to-nearest, no contraction:
//   e   = eps_u + g * (eps_c - eps_u)                     ROWS 2 (rows_per_image; 1: e = eps_u)
//   e   = (e_u + g * (e_t - e_i)) + gi * (e_i - e_u)      ROWS 3 (InstructPix2Pix: row blocks e_t, e_i, e_u in that order)
//   x'  = (a*x + b*e) + c*n                               ORDER 1; NOISE 0: a*x + b*e;  (a, b, c, s_next) = coef[*step]
//   x0  = u*x + v*e,  x' = A*x + B*x0 [+ D*hist]          ORDER 2; (u, v, A, B1, B2, D2, s_next, 0) = coef8[*step]
//   x'' = (1 - m)*(p*z + q*n0) + m*x'                     MASK 1, 2; (p, q) = blend[*step], m = mask[i / channels]
//   in  = f16_rn(x'' * s_next)                            written to every UNet row of the image; x'' stored to x
// A mode's operands are read only by the instantiations of that mode; the six mixdq_sampler_step* entry points fill
// one operand set (StepArgs), check it (check_step) and launch (launch_step), which picks the instantiation.
// mixdq_sampler_step3 is the one entry point of ROWS 3: it takes the whole operand set flat (set_flat), a mode's operands
// null where the mode is off.  The two-row blocks are (unconditional, conditional); the three-row blocks follow diffusers'
// InstructPix2Pix pipelines: block 0 text + image, block 1 image only, block 2 neither.
//
// ORDER 1 -- Euler, Euler-ancestral, DDIM and LCM with an epsilon-predicting model -- is one affine map with per-step
// scalars.  ORDER 2 (DPM-Solver++ 2M, mixdq_sampler_step_2m[_masked]) is NOT an affine map of (x, eps, noise): a
// second-order step also reads the previous step's data prediction.  That one value per element is the only state a
// multistep solver adds; it lives in a caller-owned FP32 buffer `hist`, read on second-order steps and rewritten on
// every step, with the index of the run's first step in a device int beside the step index.  These kinds add no noise:
// ORDER 2 exists with NOISE 0 only.
//
// NOISE: 0 none; 1 read from a buffer; 2 and 3 (mixdq_sampler_step[_masked]_rng) computed in registers --
// Philox4x32-10 keyed by the image's seed, counter (element / 4, *step, stream 1), then Box-Muller
// (include/mixdq_math.h: mixdq_rng_*) -- so a stochastic schedule needs no [n_steps, ...] noise buffer and a captured
// graph serves every seed (the seeds are read from device memory).  mixdq_randn_f32 fills a buffer by the same rule
// (the start noise, the VAE posterior's), mixdq_rng_normals_from_bits is the words-to-normals map alone, for tests.
//
// MASK (inpainting, the *_masked entry points): 0 none; 1 channels == 4; 2 any channel count.  Three more FP32 reads
// per element (z, n0 as 16-byte loads; the mask one value per latent pixel); the blend touches x and the UNet input,
// never `hist`.
//
// HBM-bound and small (SDXL at 1024 px: 65 536 elements per image): elementwise over storage, 8 elements per lane
// per pass -- 16-byte accesses on the FP16 tensors, two on the FP32 ones -- and a scalar tail for n % 8 elements.
//
// The step index is read by every workgroup of the step launch and advanced by the launch BEHIND it on the same
// stream (sampler_advance_kernel, one thread): launches of one stream run in order, so no workgroup of the step
// can read the index after it moved, without any in-launch ticket, fence or counter to re-initialise.
#include "sampler_step.h"

namespace mixdq {
namespace {

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

// `table` is coef (ORDER 1) or coef8 (ORDER 2); first_p: ORDER 2; blend: MASK 1, 2; the rest as sampler_step.h says.
template <int ROWS, int ORDER, int NOISE, int MASK>
__global__ __launch_bounds__(256) void sampler_step_kernel(
    float* __restrict__ x, const __half* __restrict__ eps, __half* __restrict__ in, const float* __restrict__ table,
    const int* __restrict__ step_p, int n_steps, float g, float gi, int64_t n, int64_t row_stride,
    const float* __restrict__ noise,
    int64_t noise_stride, const uint64_t* __restrict__ seeds, int64_t n_image, float* __restrict__ hist,
    const int* __restrict__ first_p, const float* __restrict__ z, const float* __restrict__ noise0,
    const float* __restrict__ mask, int channels, const float* __restrict__ blend) {
  static_assert(ORDER == 1 || (ORDER == 2 && NOISE == 0), "the multistep kinds add no noise");
  const int step = *step_p;
  if (step < 0 || step >= n_steps) return;        // replayed past the table: nothing is read or written
  StepRow k = {};
  step_row<ORDER, MASK>(k, table, first_p, blend, step, g, gi);
  const float* nz = NOISE == 1 ? noise + (int64_t)step * noise_stride : nullptr;
  const int64_t nvec = n >> 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    StepPass8 p = {};
    step_load8<ROWS, ORDER, NOISE, MASK>(p, k, step, i << 3, x, eps, row_stride, nz, seeds, n_image, hist, z, noise0, mask,
                                         channels);
#pragma unroll
    for (int j = 0; j < 8; ++j) step_elem<ROWS, ORDER, NOISE, MASK, false>(p, k, 1.0f, j);
    step_store8<ROWS, ORDER>(p, k, i << 3, x, in, row_stride, hist);
  }
  // tail (n % 8 elements), by the first threads of block 0
  const int64_t t = (nvec << 3) + threadIdx.x;
  if (blockIdx.x == 0 && t < n)
    step_at<ROWS, ORDER, NOISE, MASK, false>(k, 1.0f, step, t, x, eps, in, row_stride, nz, seeds, n_image, hist, z, noise0,
                                             mask, channels);
}

// Check, launch the instantiation the operand set asks for, then the advance.  n == 0 launches the advance alone.
int launch_step(const StepArgs& a, mixdq_stream_t stream_) {
  const int bad = check_step(a);
  if (bad != MIXDQ_OK) return bad;
  hipStream_t stream = (hipStream_t)stream_;
  if (a.n > 0) {
    const int blocks = grid_blocks(a.n >> 3);
    with_step_modes<1, 2, 3>(a, [&](auto rows, auto order, auto noise, auto mask) {
      sampler_step_kernel<decltype(rows)::value, decltype(order)::value, decltype(noise)::value, decltype(mask)::value>
          <<<blocks, 256, 0, stream>>>(a.x, (const __half*)a.eps_f16, (__half*)a.in_f16, a.table, a.step, a.n_steps,
                                       a.guidance, a.image_guidance, a.n, a.row_stride, a.noise, a.noise_stride, a.seeds,
                                       a.n_image, a.hist, a.first, a.z, a.noise0, a.mask, a.channels, a.blend);
    });
    if (hipGetLastError() != hipSuccess) return MIXDQ_ERR_LAUNCH;
  }
  sampler_advance_kernel<<<1, 1, 0, stream>>>(a.t_table, a.n_steps, a.step, a.timestep);
  return launch_status();
}

}  // namespace
}  // namespace mixdq

using namespace mixdq;

extern "C" int mixdq_sampler_step(float* x, const void* eps_f16, void* in_f16, const float* noise_or_null,
                                  int64_t noise_stride, const float* coef, const float* t_table, int n_steps,
                                  int* step, float* timestep, float guidance, int64_t n, int rows_per_image,
                                  int64_t row_stride, mixdq_stream_t stream_) {
  StepArgs a = {x, eps_f16, in_f16, coef, t_table, n_steps, step, timestep, guidance, n, rows_per_image, row_stride};
  a.noise = noise_or_null, a.noise_stride = noise_stride;
  return launch_step(a, stream_);
}

extern "C" int mixdq_sampler_step_masked(float* x, const void* eps_f16, void* in_f16, const float* noise_or_null,
                                         int64_t noise_stride, const float* coef, const float* t_table, int n_steps,
                                         int* step, float* timestep, float guidance, int64_t n, int rows_per_image,
                                         int64_t row_stride, const float* z, const float* noise0, const float* mask,
                                         int channels, const float* blend, mixdq_stream_t stream_) {
  StepArgs a = {x, eps_f16, in_f16, coef, t_table, n_steps, step, timestep, guidance, n, rows_per_image, row_stride};
  a.noise = noise_or_null, a.noise_stride = noise_stride;
  a.set_masked(z, noise0, mask, channels, blend);
  return launch_step(a, stream_);
}

// ---- noise made on the device ------------------------------------------------------------------------------------------
extern "C" int mixdq_randn_f32(float* out, int B, int64_t n_image, const uint64_t* seeds_device, uint32_t rstream,
                               uint32_t step, mixdq_stream_t stream_) {
  if (!out || !seeds_device || B < 0 || n_image < 1) return MIXDQ_ERR_INVALID_ARG;
  const bool vec = n_image % 4 == 0;
  if ((uintptr_t)out % (vec ? 16 : 4) || (uintptr_t)seeds_device % 8) return MIXDQ_ERR_ALIGNMENT;
  if (B == 0) return MIXDQ_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t qpi = (n_image + 3) / 4, total = qpi * B;
  const int blocks = grid_blocks(total);
  if (vec) randn_kernel<true><<<blocks, 256, 0, stream>>>(out, n_image, qpi, total, seeds_device, rstream, step);
  else randn_kernel<false><<<blocks, 256, 0, stream>>>(out, n_image, qpi, total, seeds_device, rstream, step);
  return launch_status();
}

extern "C" int mixdq_rng_normals_from_bits(const uint32_t* r, float* z, int64_t n_quads, mixdq_stream_t stream_) {
  if (!r || !z || n_quads < 0) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)r % 16 || (uintptr_t)z % 16) return MIXDQ_ERR_ALIGNMENT;
  if (n_quads == 0) return MIXDQ_OK;
  normals_from_bits_kernel<<<grid_blocks(n_quads), 256, 0, (hipStream_t)stream_>>>(r, z, n_quads);
  return launch_status();
}

extern "C" int mixdq_sampler_step_rng(float* x, const void* eps_f16, void* in_f16, const uint64_t* seeds,
                                      int64_t n_image, const float* coef, const float* t_table, int n_steps, int* step,
                                      float* timestep, float guidance, int64_t n, int rows_per_image, int64_t row_stride,
                                      mixdq_stream_t stream_) {
  StepArgs a = {x, eps_f16, in_f16, coef, t_table, n_steps, step, timestep, guidance, n, rows_per_image, row_stride};
  a.rng = true, a.seeds = seeds, a.n_image = n_image;
  return launch_step(a, stream_);
}

extern "C" int mixdq_sampler_step_masked_rng(float* x, const void* eps_f16, void* in_f16, const uint64_t* seeds,
                                             int64_t n_image, const float* coef, const float* t_table, int n_steps,
                                             int* step, float* timestep, float guidance, int64_t n, int rows_per_image,
                                             int64_t row_stride, const float* z, const float* noise0, const float* mask,
                                             int channels, const float* blend, mixdq_stream_t stream_) {
  StepArgs a = {x, eps_f16, in_f16, coef, t_table, n_steps, step, timestep, guidance, n, rows_per_image, row_stride};
  a.rng = true, a.seeds = seeds, a.n_image = n_image;
  a.set_masked(z, noise0, mask, channels, blend);
  return launch_step(a, stream_);
}

// ---- the multistep kinds: `hist` and `first` beside the base operands, coef8 as the table -----------------------------
extern "C" int mixdq_sampler_step_2m(float* x, const void* eps_f16, void* in_f16, float* hist, const float* coef8,
                                     const float* t_table, int n_steps, int* step, const int* first, float* timestep,
                                     float guidance, int64_t n, int rows_per_image, int64_t row_stride,
                                     mixdq_stream_t stream_) {
  StepArgs a = {x, eps_f16, in_f16, coef8, t_table, n_steps, step, timestep, guidance, n, rows_per_image, row_stride};
  a.multistep = true, a.hist = hist, a.first = first;
  return launch_step(a, stream_);
}

extern "C" int mixdq_sampler_step_2m_masked(float* x, const void* eps_f16, void* in_f16, float* hist, const float* coef8,
                                            const float* t_table, int n_steps, int* step, const int* first,
                                            float* timestep, float guidance, int64_t n, int rows_per_image,
                                            int64_t row_stride, const float* z, const float* noise0, const float* mask,
                                            int channels, const float* blend, mixdq_stream_t stream_) {
  StepArgs a = {x, eps_f16, in_f16, coef8, t_table, n_steps, step, timestep, guidance, n, rows_per_image, row_stride};
  a.multistep = true, a.hist = hist, a.first = first;
  a.set_masked(z, noise0, mask, channels, blend);
  return launch_step(a, stream_);
}

// ---- three rows per image (InstructPix2Pix): the whole operand set flat, a mode's operands null where it is off --------
extern "C" int mixdq_sampler_step3(float* x, const void* eps_f16, void* in_f16, const float* table, int table_width,
                                   const float* t_table, int n_steps, int* step, float* timestep, float guidance,
                                   float image_guidance, int64_t n, int64_t row_stride, const float* noise_or_null,
                                   int64_t noise_stride, const uint64_t* seeds_or_null, int64_t n_image,
                                   float* hist_or_null, const int* first_or_null, const float* z, const float* noise0,
                                   const float* mask, int channels, const float* blend, mixdq_stream_t stream_) {
  StepArgs a = {x, eps_f16, in_f16, table, t_table, n_steps, step, timestep, guidance, n, 3, row_stride};
  a.three = true, a.image_guidance = image_guidance;
  const int bad = set_flat(a, table_width, noise_or_null, noise_stride, seeds_or_null, n_image, hist_or_null, first_or_null,
                           z, noise0, mask, channels, blend);
  if (bad != MIXDQ_OK) return bad;
  return launch_step(a, stream_);
}
