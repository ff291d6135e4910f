// Guidance rescale in the device-side sampling loop (mixdq_sampler_step_rescaled): the sampler step of sampler.hip with
// the guided model output multiplied, per image, by r = 1 + phi * (sqrt(M2_t / M2_e) - 1) -- the ratio of the standard
// deviations of the text-conditioned and the guided output over all of the image's elements (Lin et al., "Common
// diffusion noise schedules and sample steps are flawed"; diffusers' guidance_rescale).  No reference counterpart.
// The arithmetic, rounding by rounding and sum by sum, is include/mixdq_math.h (mixdq_rescale_*); its numpy
// restatement is tests/rescale_ref.py.
//
// r is known only after EVERY element of the image was read, so a step is three launches on one (chunk, image) grid --
// chunk: MIXDQ_RESCALE_CHUNK = 2048 consecutive storage elements of one image, 256 lanes x 8; blockIdx.y the image:
//   sampler_rescale_stats_kernel<ROWS, VEC>            per chunk (mean_t, M2_t, mean_e, M2_e) -> workspace; one pass of
//                                                      FP16 loads over the 2 or 3 row blocks, both passes of the
//                                                      two-pass variance over values held in registers
//   sampler_step_rescaled_kernel<ROWS, ORDER, NOISE, MASK>   combines the image's chunks in chunk order (Chan's update,
//                                                      ~32 dependent updates at SDXL's latent size) in its prologue --
//                                                      every workgroup of the image redundantly, the same bits -- then
//                                                      the step's body (sampler_step.h) with e * r in the place of e
//   sampler_advance_kernel                             the sibling's
// Stream order is the only synchronisation (the comment at the top of sampler.hip): no atomics, no tickets, no block
// that finalizes.  The grids are exact -- one workgroup per chunk, nothing capped, no grid-stride loop -- and no
// element index is divided by n_image outside the sibling's noise helpers.  MIXDQ_RESCALE_COMBINE_LAUNCH=1 moves the
// combine into a launch of its own between the two (sampler_rescale_factor_kernel, one lane per image, r[B] behind
// the chunk statistics in the workspace): the alternative the choice was measured against.
//
// VEC (n_image % 8 == 0): every lane's 8 elements are 16-byte aligned in every tensor and a chunk holds whole lanes;
// otherwise element by element, up to 8 per lane (any n_image, any tail).  The workspace is the caller's
// (mixdq_sampler_rescale_workspace_floats): nothing is allocated here, a captured graph replays it as it is.
#include "sampler_step.h"

namespace mixdq {
namespace {

constexpr int kChunk = MIXDQ_RESCALE_CHUNK;

// The count of chunk `c` of an image, and how many of a lane's 8 elements lie inside it.
__device__ __forceinline__ int chunk_count(int64_t n_image, int64_t c) {
  const int64_t left = n_image - c * kChunk;       // >= 1: the grid has ceil(n_image / kChunk) chunks
  return left < kChunk ? (int)left : kChunk;
}
__device__ __forceinline__ int lane_count(int count) { return min(max(count - 8 * (int)threadIdx.x, 0), 8); }

// S of include/mixdq_math.h, for two tensors at once, from every lane's partial: the wave's balanced tree over
// lane ^ 1, 2, .. 32, then the four waves in order.  `red`: 8 floats of LDS; every lane returns with the sums.
__device__ __forceinline__ void chunk_sum2(float pa, float pb, float* red, float* sa, float* sb) {
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    pa = MIXDQ_ADD_RN(pa, __shfl_xor(pa, k));
    pb = MIXDQ_ADD_RN(pb, __shfl_xor(pb, k));
  }
  __syncthreads();                                 // (the previous call's sums have been read)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = pa, red[4 + (threadIdx.x >> 6)] = pb;
  __syncthreads();
  *sa = MIXDQ_ADD_RN(MIXDQ_ADD_RN(MIXDQ_ADD_RN(red[0], red[1]), red[2]), red[3]);
  *sb = MIXDQ_ADD_RN(MIXDQ_ADD_RN(MIXDQ_ADD_RN(red[4], red[5]), red[6]), red[7]);
}

template <int ROWS, bool VEC>
__global__ __launch_bounds__(256) void sampler_rescale_stats_kernel(const __half* __restrict__ eps,
                                                                    const int* __restrict__ step_p, int n_steps, float g,
                                                                    float gi, int64_t n_image, int64_t row_stride,
                                                                    float* __restrict__ ws) {
  static_assert(ROWS == 2 || ROWS == 3, "guidance rescale compares two outputs of one image");
  __shared__ float red[8];
  const int step = *step_p;
  if (step < 0 || step >= n_steps) return;         // replayed past the table: nothing is read or written
  const int count = chunk_count(n_image, blockIdx.x), mine = lane_count(count);
  const int64_t o = (int64_t)blockIdx.y * n_image + (int64_t)blockIdx.x * kChunk + 8 * threadIdx.x;
  float t[8] = {}, e[8] = {};
  if (VEC) {
    if (mine == 8) {                               // n_image % 8 == 0: a lane has all 8 or none
      const Half8 e0 = *reinterpret_cast<const Half8*>(eps + o);
      const Half8 e1 = *reinterpret_cast<const Half8*>(eps + row_stride + o);
      Half8 e2 = e0;
      if (ROWS == 3) e2 = *reinterpret_cast<const Half8*>(eps + 2 * row_stride + o);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        t[j] = ROWS == 3 ? half_at(e0, j) : half_at(e1, j);
        e[j] = step_guided<ROWS>(half_at(e0, j), half_at(e1, j), half_at(e2, j), g, gi);
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < mine) {                              // o + j < (blockIdx.y + 1) * n_image <= n
        const float e0 = __half2float(eps[o + j]), e1 = __half2float(eps[row_stride + o + j]);
        const float e2 = ROWS == 3 ? __half2float(eps[2 * row_stride + o + j]) : e0;
        t[j] = ROWS == 3 ? e0 : e1;
        e[j] = step_guided<ROWS>(e0, e1, e2, g, gi);
      }
    }
  }
  float sum_t, sum_e, m2_t, m2_e;
  chunk_sum2(mixdq_rescale_lane_sum(t), mixdq_rescale_lane_sum(e), red, &sum_t, &sum_e);
  const float mean_t = MIXDQ_DIV_RN(sum_t, (float)count), mean_e = MIXDQ_DIV_RN(sum_e, (float)count);
#pragma unroll
  for (int j = 0; j < 8; ++j) {                    // the second pass, over the same registers; absent elements add +0
    t[j] = j < mine ? mixdq_rescale_sqdev(t[j], mean_t) : 0.0f;
    e[j] = j < mine ? mixdq_rescale_sqdev(e[j], mean_e) : 0.0f;
  }
  chunk_sum2(mixdq_rescale_lane_sum(t), mixdq_rescale_lane_sum(e), red, &m2_t, &m2_e);
  if (threadIdx.x == 0)
    *reinterpret_cast<float4*>(ws + 4 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x)) =
        make_float4(mean_t, m2_t, mean_e, m2_e);
}

// r of image b from its `chunks` workspace rows, in chunk order (mixdq_rescale_combine): uniform over the caller's lanes.
__device__ __forceinline__ float image_factor(const float* __restrict__ ws, int64_t b, int64_t chunks, int64_t n_image,
                                              float phi) {
  const float4* __restrict__ rows = reinterpret_cast<const float4*>(ws) + b * chunks;
  float mean_t = 0.0f, m2_t = 0.0f, mean_e = 0.0f, m2_e = 0.0f;
  int64_t seen = 0;
  for (int64_t c = 0; c < chunks; ++c) {
    const float4 v = rows[c];
    const int64_t k = chunk_count(n_image, c);
    mixdq_rescale_combine(seen, k, v.x, v.y, &mean_t, &m2_t);
    mixdq_rescale_combine(seen, k, v.z, v.w, &mean_e, &m2_e);
    seen += k;
  }
  return mixdq_rescale_factor(m2_t, m2_e, phi, n_image);
}

// MIXDQ_RESCALE_COMBINE_LAUNCH=1: one lane per image, r[b] behind the statistics.
__global__ __launch_bounds__(64) void sampler_rescale_factor_kernel(float* __restrict__ ws,
                                                                    const int* __restrict__ step_p, int n_steps,
                                                                    int64_t images, int64_t chunks, int64_t n_image,
                                                                    float phi) {
  const int step = *step_p;
  if (step < 0 || step >= n_steps) return;
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b < images) ws[4 * images * chunks + b] = image_factor(ws, b, chunks, n_image, phi);
}

// The step's body (sampler_step.h) on chunk blockIdx.x of image blockIdx.y with e * r in the place of the guided e; this
// kernel's own are the chunk arithmetic, r, and which lanes take the 8-element pass.  `factors`: r[images] where
// the factor launch ran, else null: the combine runs here.  Operands of a mode as in the sibling.
template <int ROWS, int ORDER, int NOISE, int MASK>
__global__ __launch_bounds__(256) void sampler_step_rescaled_kernel(
    float* __restrict__ x, const __half* __restrict__ eps, __half* __restrict__ in, const float* __restrict__ table,
    const int* __restrict__ step_p, int n_steps, float g, float gi, float phi, int64_t row_stride,
    const float* __restrict__ noise, int64_t noise_stride, const uint64_t* __restrict__ seeds, int64_t n_image,
    float* __restrict__ hist, const int* __restrict__ first_p, const float* __restrict__ z,
    const float* __restrict__ noise0, const float* __restrict__ mask, int channels, const float* __restrict__ blend,
    const float* __restrict__ ws, const float* __restrict__ factors) {
  static_assert(ROWS == 2 || ROWS == 3, "guidance rescale compares two outputs of one image");
  static_assert(ORDER == 1 || (ORDER == 2 && NOISE == 0), "the multistep kinds add no noise");
  const int step = *step_p;
  if (step < 0 || step >= n_steps) return;         // replayed past the table: nothing is read or written
  StepRow k = {};
  step_row<ORDER, MASK>(k, table, first_p, blend, step, g, gi);
  const float r = factors ? factors[blockIdx.y] : image_factor(ws, blockIdx.y, gridDim.x, n_image, phi);
  const float* nz = NOISE == 1 ? noise + (int64_t)step * noise_stride : nullptr;
  const int mine = lane_count(chunk_count(n_image, blockIdx.x));
  const int64_t o = (int64_t)blockIdx.y * n_image + (int64_t)blockIdx.x * kChunk + 8 * threadIdx.x;
  if (mine == 0) return;
  // NOISE 2 exists for n_image % 8 == 0 only and NOISE 3 for the rest (the entry point's choice, as the sibling's)
  if (NOISE != 3 && (NOISE == 2 || n_image % 8 == 0)) {
    StepPass8 p = {};
    step_load8<ROWS, ORDER, NOISE, MASK>(p, k, step, o, x, eps, row_stride, nz, seeds, n_image, hist, z, noise0, mask,
                                         channels);
#pragma unroll
    for (int j = 0; j < 8; ++j) step_elem<ROWS, ORDER, NOISE, MASK, true>(p, k, r, j);
    step_store8<ROWS, ORDER>(p, k, o, x, in, row_stride, hist);
  } else if constexpr (NOISE != 2) {
    for (int j = 0; j < mine; ++j)                 // element by element; o + j < (blockIdx.y + 1) * n_image <= n
      step_at<ROWS, ORDER, NOISE, MASK, true>(k, r, step, o + j, x, eps, in, row_stride, nz, seeds, n_image, hist, z,
                                              noise0, mask, channels);
  }
}

int64_t chunks_of(int64_t n_image) { return (n_image + kChunk - 1) / kChunk; }

}  // namespace
}  // namespace mixdq

using namespace mixdq;

extern "C" size_t mixdq_sampler_rescale_workspace_floats(int64_t n, int64_t n_image) {
  if (n < 0 || n_image < 1 || n % n_image) return 0;
  const int64_t images = n / n_image;
  return (size_t)(4 * images * chunks_of(n_image) + images);
}

extern "C" int mixdq_sampler_step_rescaled(float* x, const void* eps_f16, void* in_f16, const float* table,
                                           int table_width, const float* t_table, int n_steps, int* step,
                                           float* timestep, float guidance, float image_guidance, float rescale,
                                           int rows_per_image, int64_t n, int64_t n_image, int64_t row_stride,
                                           float* workspace, const float* noise_or_null, int64_t noise_stride,
                                           const uint64_t* seeds_or_null, float* hist_or_null, const int* first_or_null,
                                           const float* z, const float* noise0, const float* mask, int channels,
                                           const float* blend, mixdq_stream_t stream_) {
  if (rows_per_image != 2 && rows_per_image != 3) return MIXDQ_ERR_INVALID_ARG;
  StepArgs a = {x, eps_f16, in_f16, table, t_table, n_steps, step, timestep, guidance, n, rows_per_image, row_stride};
  a.three = rows_per_image == 3, a.image_guidance = image_guidance;
  int bad = set_flat(a, table_width, noise_or_null, noise_stride, seeds_or_null, n_image, hist_or_null, first_or_null, z,
                     noise0, mask, channels, blend);
  if (bad != MIXDQ_OK) return bad;
  a.n_image = n_image;                             // (with or without seeds: the statistics are per image)
  bad = check_step(a);
  if (bad != MIXDQ_OK) return bad;
  if (!(rescale >= 0.0f && rescale <= 1.0f)) return MIXDQ_ERR_INVALID_ARG;      // (NaN compares false)
  if (n_image < 1 || n % n_image || !workspace) return MIXDQ_ERR_INVALID_ARG;
  const int64_t images = n / n_image, chunks = chunks_of(n_image);
  if (images > 65535 || chunks > INT32_MAX) return MIXDQ_ERR_INVALID_ARG;       // the grid's y and x extents
  if ((uintptr_t)workspace % 16) return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  if (n > 0) {
    static const bool combine_launch = env_flag("MIXDQ_RESCALE_COMBINE_LAUNCH", false);
    const dim3 grid((unsigned)chunks, (unsigned)images);
    const __half* eps = (const __half*)eps_f16;
    with_constant<2, 3>(rows_per_image, [&](auto rows) {
      with_bool(n_image % 8 == 0, [&](auto vec) {
        sampler_rescale_stats_kernel<decltype(rows)::value, decltype(vec)::value><<<grid, 256, 0, stream>>>(
            eps, step, n_steps, guidance, image_guidance, n_image, row_stride, workspace);
      });
    });
    if (hipGetLastError() != hipSuccess) return MIXDQ_ERR_LAUNCH;
    const float* factors = nullptr;
    if (combine_launch) {
      factors = workspace + 4 * images * chunks;
      sampler_rescale_factor_kernel<<<(unsigned)((images + 63) / 64), 64, 0, stream>>>(workspace, step, n_steps, images,
                                                                                        chunks, n_image, rescale);
      if (hipGetLastError() != hipSuccess) return MIXDQ_ERR_LAUNCH;
    }
    with_step_modes<2, 3>(a, [&](auto rows, auto order, auto noise, auto mask) {
      sampler_step_rescaled_kernel<decltype(rows)::value, decltype(order)::value, decltype(noise)::value,
                                   decltype(mask)::value><<<grid, 256, 0, stream>>>(
          x, eps, (__half*)in_f16, table, step, n_steps, guidance, image_guidance, rescale, row_stride, a.noise,
          a.noise_stride, a.seeds, n_image, a.hist, a.first, a.z, a.noise0, a.mask, a.channels, a.blend, workspace, factors);
    });
    if (hipGetLastError() != hipSuccess) return MIXDQ_ERR_LAUNCH;
  }
  sampler_advance_kernel<<<1, 1, 0, stream>>>(t_table, n_steps, step, timestep);
  return launch_status();
}
