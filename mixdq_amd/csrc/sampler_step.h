// What the sampler step's translation units share (sampler.hip, sampler_rescale.hip): the noise and mask operands of an
// 8-element pass, the scalars of a launch (StepRow) and the per-element function (step_one), the advance launch, and
// the operand set of a step with its checks (StepArgs, check_step).  Everything is in an unnamed namespace: each unit
// has its own copy, and a kernel keeps the symbol name it has in its unit.
#pragma once
#include "common.h"
#include "../../include/mixdq_math.h"

namespace mixdq {
namespace {

// NOISE, the step kernel's noise mode: 0 none, 1 read from a buffer, 2 and 3 computed in registers (mixdq_rng_*,
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

// The noise of the 8-element pass at storage element o; NOISE 0 leaves ns alone.
template <int NOISE>
__device__ __forceinline__ void noise8(const float* __restrict__ nz, const uint64_t* __restrict__ seeds, int64_t n_image,
                                       int64_t o, uint32_t step, float ns[8]) {
  if constexpr (NOISE == 1) load8(nz + o, ns);
  if constexpr (NOISE >= 2) rng_noise8<NOISE == 2>(seeds, n_image, o, step, ns);
}

// The mask values of the 8-element pass at storage element o (o % 8 == 0): element i of the (channels-last) storage
// belongs to mask entry i / channels.  MASK 1: channels == 4, the pass covers exactly two latent pixels; MASK 2: the
// quotient and remainder of the pass's first element are divided out once and carried along.
template <int MASK>
__device__ __forceinline__ void mask8(const float* __restrict__ mask, int channels, int64_t o, float ms[8]) {
  if constexpr (MASK == 1) {
    const float m0 = mask[o >> 2], m1 = mask[(o >> 2) + 1];
#pragma unroll
    for (int j = 0; j < 8; ++j) ms[j] = j < 4 ? m0 : m1;
  } else {
    int64_t q = o / channels;                      // o + j < n and n % channels == 0: q stays below n / channels
    int r = (int)(o - q * channels);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ms[j] = mask[q];
      if (++r == channels) { r = 0; ++q; }
    }
  }
}

// The scalars of one launch: the guidance scale (ROWS 3: and the image guidance scale gi) and row *step of the tables.  ORDER 1: (a, b, c, s_next) = coef[*step].
// ORDER 2: a = A, d = D2 and b = B2 on a second-order step, B1 on a first-order one.  Which order a step takes depends
// on the table and on two device scalars only -- the first executed step of a run (*step == *first) and a row with
// D2 == 0 are first-order -- so `second` is uniform over the launch.  MASK: (p, q) = blend[*step].
struct StepRow {
  float g, gi, a, b, c, u, v, d, s_next, p, q;
  bool second;
};

// One element: guidance, the update, the blend.  (e0, e1, e2) are the element's values in the row blocks -- ROWS 1: e0;
// ROWS 2: (eps_u, eps_c); ROWS 3: (e_t, e_i, e_u).  n, h and (z, n0, m) are operands of NOISE != 0, of a second-order
// step and of MASK != 0 only; ORDER 2 hands the data prediction (the next step's h, unblended) back in *x0_out.
template <int ROWS, int ORDER, int NOISE, int MASK>
__device__ __forceinline__ float step_one(const StepRow& k, float x, float e0, float e1, float e2, float n, float h,
                                          float z, float n0, float m, float* x0_out) {
  const float e = ROWS == 3   ? mixdq_sampler_guided_eps3(e0, e1, e2, k.g, k.gi)
                  : ROWS == 2 ? mixdq_sampler_guided_eps(e0, e1, k.g)
                              : e0;
  float y;
  if constexpr (ORDER == 1) {
    y = NOISE ? mixdq_sampler_update_noise(x, e, n, k.a, k.b, k.c) : mixdq_sampler_update(x, e, k.a, k.b);
  } else {
    const float x0 = mixdq_sampler_x0(x, e, k.u, k.v);
    *x0_out = x0;
    // both computed, one selected: a branch per element would cut the 8-element pass into blocks (more registers)
    const float y1 = mixdq_sampler_update(x, x0, k.a, k.b), y2 = mixdq_sampler_update_2m(x, x0, h, k.a, k.b, k.d);
    y = k.second ? y2 : y1;
  }
  return MASK ? mixdq_sampler_blend(y, z, n0, m, k.p, k.q) : y;
}

// Behind the step on the same stream: the timestep of the NEXT UNet forward, and the index moves on.
__global__ void sampler_advance_kernel(const float* __restrict__ t_table, int n_steps, int* step_p, float* timestep) {
  const int step = *step_p;
  if (step < 0 || step >= n_steps) return;
  *timestep = t_table[step + 1];
  *step_p = step + 1;
}

// The operand set of one step.  The first block is every entry point's (`table`: coef, or coef8 where multistep);
// an entry point sets `rng` / `multistep` / `masked` and the operands of that mode, which are checked and read only then.
struct StepArgs {
  float* x;
  const void *eps_f16;
  void* in_f16;
  const float *table, *t_table;
  int n_steps;
  int* step;
  float* timestep;
  float guidance;
  int64_t n;
  int rows_per_image;
  int64_t row_stride;
  float image_guidance = 0.0f;                     // rows_per_image == 3
  bool three = false;                              // mixdq_sampler_step3: the only entry point that takes three rows
  const float* noise = nullptr;                    // the plain entry points' noise_or_null
  int64_t noise_stride = 0;
  bool rng = false, multistep = false, masked = false;
  const uint64_t* seeds = nullptr;
  int64_t n_image = 0;
  float* hist = nullptr;
  const int* first = nullptr;
  const float *z = nullptr, *noise0 = nullptr, *mask = nullptr, *blend = nullptr;
  int channels = 1;

  void set_masked(const float* z_, const float* noise0_, const float* mask_, int channels_, const float* blend_) {
    masked = true, z = z_, noise0 = noise0_, mask = mask_, channels = channels_, blend = blend_;
  }
};

// The argument checks of every entry point, in one order: the base operands, then those of rng, multistep, masked.
int check_step(const StepArgs& a) {
  if (!a.x || !a.eps_f16 || !a.in_f16 || !a.table || !a.t_table || !a.step || !a.timestep) return MIXDQ_ERR_INVALID_ARG;
  if (a.n < 0 || a.n_steps < 1 || (a.three ? a.rows_per_image != 3 : a.rows_per_image != 1 && a.rows_per_image != 2))
    return MIXDQ_ERR_INVALID_ARG;
  if (a.rows_per_image >= 2 && a.row_stride < a.n) return MIXDQ_ERR_INVALID_ARG;  // the row blocks would overlap
  if (a.noise && a.noise_stride < a.n) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)a.x % 16 || (uintptr_t)a.eps_f16 % 16 || (uintptr_t)a.in_f16 % 16 || (uintptr_t)a.table % 16 ||
      (uintptr_t)a.noise % 16 || (uintptr_t)a.t_table % 4 || (uintptr_t)a.step % 4 || (uintptr_t)a.timestep % 4)
    return MIXDQ_ERR_ALIGNMENT;
  if ((a.rows_per_image >= 2 && a.row_stride % 8) || (a.noise && a.noise_stride % 4)) return MIXDQ_ERR_ALIGNMENT;
  if (a.rng) {
    if (!a.seeds || a.n_image < 1 || a.n % a.n_image) return MIXDQ_ERR_INVALID_ARG;
    if ((uintptr_t)a.seeds % 8) return MIXDQ_ERR_ALIGNMENT;
  }
  if (a.multistep) {
    if (!a.hist || !a.first) return MIXDQ_ERR_INVALID_ARG;
    if (a.hist < a.x + a.n && a.x < a.hist + a.n) return MIXDQ_ERR_INVALID_ARG;  // the history is a buffer of its own
    if ((uintptr_t)a.hist % 16 || (uintptr_t)a.first % 4) return MIXDQ_ERR_ALIGNMENT;
  }
  if (a.masked) {
    if (!a.z || !a.noise0 || !a.mask || !a.blend || a.channels < 1 || a.n % a.channels) return MIXDQ_ERR_INVALID_ARG;
    if ((uintptr_t)a.z % 16 || (uintptr_t)a.noise0 % 16 || (uintptr_t)a.mask % 4 || (uintptr_t)a.blend % 8)
      return MIXDQ_ERR_ALIGNMENT;
  }
  return MIXDQ_OK;
}

}  // namespace
}  // namespace mixdq
