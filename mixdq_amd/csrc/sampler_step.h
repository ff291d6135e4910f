// What the sampler step's translation units share (sampler.hip, sampler_rescale.hip).  Device side: the noise and mask
// operands of an 8-element pass, the scalars of a launch (StepRow, step_row), the per-element functions (step_guided,
// step_update) and the step's body, which both step kernels call -- an 8-element pass (step_load8, step_elem,
// step_store8) and a single element (step_at); the advance launch.  Host side: the operand set of a step with its
// checks (StepArgs, check_step), the flat entry points' decoder (set_flat), the mode dispatch (with_step_modes).
// Everything is in an unnamed namespace: each unit has its own copy, and a kernel keeps the symbol name it has in its unit.
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

// Row `step` of the tables into a launch's scalars; `first_p` is read by ORDER 2 only, `blend` by MASK != 0 only.
template <int ORDER, int MASK>
__device__ __forceinline__ void step_row(StepRow& k, const float* table, const int* first_p, const float* blend, int step,
                                         float g, float gi) {
  k.g = g, k.gi = gi;
  if constexpr (ORDER == 1) {
    const float4 r = *reinterpret_cast<const float4*>(table + 4 * (int64_t)step);
    k.a = r.x, k.b = r.y, k.c = r.z, k.s_next = r.w;
  } else {
    const float4 r0 = *reinterpret_cast<const float4*>(table + 8 * (int64_t)step);
    const float4 r1 = *reinterpret_cast<const float4*>(table + 8 * (int64_t)step + 4);
    k.u = r0.x, k.v = r0.y, k.a = r0.z, k.d = r1.y, k.s_next = r1.z;
    k.second = step > *first_p && k.d != 0.0f;
    k.b = k.second ? r1.x : r0.w;
  }
  if constexpr (MASK != 0) {
    const float2 pq = *reinterpret_cast<const float2*>(blend + 2 * (int64_t)step);
    k.p = pq.x, k.q = pq.y;
  }
}

// One element's guidance from its values in the row blocks -- ROWS 1: e0; 2: (eps_u, eps_c); 3: (e_t, e_i, e_u) ...
template <int ROWS>
__device__ __forceinline__ float step_guided(float e0, float e1, float e2, float g, float gi) {
  return ROWS == 3 ? mixdq_sampler_guided_eps3(e0, e1, e2, g, gi) : ROWS == 2 ? mixdq_sampler_guided_eps(e0, e1, g) : e0;
}

// ... and its update and blend, from the guided (or guided and rescaled) e.  n, h and (z, n0, m) are operands of NOISE
// != 0, of a second-order step and of MASK != 0 only; ORDER 2 hands x0 (the next step's h, unblended) back in *x0_out.
template <int ORDER, int NOISE, int MASK>
__device__ __forceinline__ float step_update(const StepRow& k, float x, float e, float n, float h, float z, float n0,
                                             float m, float* x0_out) {
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

// The step's body, once for both kernels, on the kernels' own operands (`table`, `blend`, `first_p` have gone into
// StepRow) -- nz, the step's block of `noise`: NOISE 1; (seeds, n_image): NOISE 2, 3; hist: ORDER 2, not read at all on a
// first-order step (it may hold anything there); (z, noise0, mask, channels): MASK 1, 2; the other instantiations never
// touch them (they are passed null).  RESCALED: e * r in the place of the guided e; r is not read otherwise.
// The 8-element pass at storage element o (o % 8 == 0, o + 8 <= n) is: StepPass8 p = {}; step_load8(p, ..); step_elem
// (p, .., j) for j = 0 .. 7, unrolled IN THE KERNEL; step_store8(p, ..).  Three calls and a struct of the caller's, not
// one function, because a helper is optimised on its own before it is inlined: as one function the pass costs the
// NOISE 3 kernels up to 14 VGPRs and three instantiations a wave of occupancy; as this, none.
struct StepPass8 {
  float xs[8], ns[8], hs[8], zs[8], is[8], ms[8], y[8], p0[8];
  Half8 e0, e1, e2;
};

// The loads of a pass: x and the row blocks are in flight while the noise is generated; then the history, the mask.
template <int ROWS, int ORDER, int NOISE, int MASK>
__device__ __forceinline__ void step_load8(StepPass8& p, const StepRow& k, int step, int64_t o,
                                           const float* __restrict__ x, const __half* __restrict__ eps, int64_t row_stride,
                                           const float* __restrict__ nz, const uint64_t* __restrict__ seeds,
                                           int64_t n_image, const float* __restrict__ hist, const float* __restrict__ z,
                                           const float* __restrict__ noise0, const float* __restrict__ mask, int channels) {
  load8(x + o, p.xs);
  p.e0 = *reinterpret_cast<const Half8*>(eps + o);
  p.e1 = p.e0, p.e2 = p.e0;
  if (ROWS >= 2) p.e1 = *reinterpret_cast<const Half8*>(eps + row_stride + o);
  if (ROWS == 3) p.e2 = *reinterpret_cast<const Half8*>(eps + 2 * row_stride + o);
  noise8<NOISE>(nz, seeds, n_image, o, (uint32_t)step, p.ns);
  if constexpr (ORDER == 2) {
    float hs[8] = {};                              // (a local, stored whole: a conditional store to p.hs costs registers)
    if (k.second) load8(hist + o, hs);
#pragma unroll
    for (int j = 0; j < 8; ++j) p.hs[j] = hs[j];
  }
  if constexpr (MASK != 0) {
    load8(z + o, p.zs);
    load8(noise0 + o, p.is);
    mask8<MASK>(mask, channels, o, p.ms);
  }
}

// Element j of the pass: p.y[j], and with ORDER 2 p.p0[j].
template <int ROWS, int ORDER, int NOISE, int MASK, bool RESCALED>
__device__ __forceinline__ void step_elem(StepPass8& p, const StepRow& k, float r, int j) {
  float e = step_guided<ROWS>(half_at(p.e0, j), half_at(p.e1, j), half_at(p.e2, j), k.g, k.gi);
  if (RESCALED) e = mixdq_sampler_rescaled(e, r);
  p.y[j] = step_update<ORDER, NOISE, MASK>(k, p.xs[j], e, p.ns[j], p.hs[j], p.zs[j], p.is[j], p.ms[j], &p.p0[j]);
}

// The stores of a pass: the history, the state, and the next FP16 input to every row block.
template <int ROWS, int ORDER>
__device__ __forceinline__ void step_store8(const StepPass8& p, const StepRow& k, int64_t o, float* __restrict__ x,
                                            __half* __restrict__ in, int64_t row_stride, float* __restrict__ hist) {
  Half8 out;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    out.w[j] = half_bits(mixdq_sampler_scaled_input(p.y[2 * j], k.s_next)) |
               (half_bits(mixdq_sampler_scaled_input(p.y[2 * j + 1], k.s_next)) << 16);
  if constexpr (ORDER == 2) store8(hist + o, p.p0);
  store8(x + o, p.y);
  *reinterpret_cast<Half8*>(in + o) = out;
  if (ROWS >= 2) *reinterpret_cast<Half8*>(in + row_stride + o) = out;
  if (ROWS == 3) *reinterpret_cast<Half8*>(in + 2 * row_stride + o) = out;
}

// The single element at storage element t (t < n): the same step with scalar accesses.
template <int ROWS, int ORDER, int NOISE, int MASK, bool RESCALED>
__device__ __forceinline__ void step_at(const StepRow& k, float r, int step, int64_t t, float* __restrict__ x,
                                        const __half* __restrict__ eps, __half* __restrict__ in, int64_t row_stride,
                                        const float* __restrict__ nz, const uint64_t* __restrict__ seeds, int64_t n_image,
                                        float* __restrict__ hist, const float* __restrict__ z,
                                        const float* __restrict__ noise0, const float* __restrict__ mask, int channels) {
  const float e0 = __half2float(eps[t]);
  const float e1 = ROWS >= 2 ? __half2float(eps[row_stride + t]) : e0;
  const float e2 = ROWS == 3 ? __half2float(eps[2 * row_stride + t]) : e0;
  float e = step_guided<ROWS>(e0, e1, e2, k.g, k.gi);
  if (RESCALED) e = mixdq_sampler_rescaled(e, r);
  float hv = 0.0f, zv = 0.0f, iv = 0.0f, mv = 0.0f, p0;
  if constexpr (ORDER == 2) {
    if (k.second) hv = hist[t];
  }
  if constexpr (MASK != 0) zv = z[t], iv = noise0[t], mv = mask[t / channels];
  const float y = step_update<ORDER, NOISE, MASK>(
      k, x[t], e, tail_noise<NOISE>(nz, seeds, n_image, t, (uint32_t)step), hv, zv, iv, mv, &p0);
  const __half h = f32_to_f16_rn(mixdq_sampler_scaled_input(y, k.s_next));
  if constexpr (ORDER == 2) hist[t] = p0;
  x[t] = y;
  in[t] = h;
  if (ROWS >= 2) in[row_stride + t] = h;
  if (ROWS == 3) in[2 * row_stride + t] = h;
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

// The flat entry points (mixdq_sampler_step3, mixdq_sampler_step_rescaled) take every mode's operands, null where the
// mode is off: the table's width and what is set say which modes are on.  Refuses modes that exclude each other.
int set_flat(StepArgs& a, int table_width, const float* noise, int64_t noise_stride, const uint64_t* seeds, int64_t n_image,
             float* hist, const int* first, const float* z, const float* noise0, const float* mask, int channels,
             const float* blend) {
  const bool two_m = table_width == 8, stochastic = noise || seeds;
  if (table_width != 4 && !two_m) return MIXDQ_ERR_INVALID_ARG;
  if ((two_m && stochastic) || (noise && seeds)) return MIXDQ_ERR_INVALID_ARG;
  if (two_m != (hist || first)) return MIXDQ_ERR_INVALID_ARG;   // (one of the pair: check_step's null check)
  a.noise = noise, a.noise_stride = noise_stride;
  if (seeds) a.rng = true, a.seeds = seeds, a.n_image = n_image;
  if (two_m) a.multistep = true, a.hist = hist, a.first = first;
  if (z || noise0 || mask || blend) a.set_masked(z, noise0, mask, channels, blend);
  return MIXDQ_OK;
}

struct StepModes { int order, noise, mask; };      // ORDER, NOISE, MASK
StepModes step_modes(const StepArgs& a) {
  return {a.multistep ? 2 : 1, a.rng ? (a.n_image % 8 == 0 ? 2 : 3) : (a.noise ? 1 : 0),
          a.masked ? (a.channels == 4 ? 1 : 2) : 0};
}

// f(rows, order, noise, mask), four std::integral_constant, for the instantiation a checked operand set asks for (rows
// among ROWS...); the combinations that do not exist (the multistep kinds add no noise) are never instantiated.
template <int... ROWS, class F>
void with_step_modes(const StepArgs& a, F&& f) {
  const StepModes m = step_modes(a);
  with_constant<ROWS...>(a.rows_per_image, [&](auto rows) {
    with_constant<1, 2>(m.order, [&](auto order) {
      with_constant<0, 1, 2, 3>(m.noise, [&](auto noise) {
        with_constant<0, 1, 2>(m.mask, [&](auto mask) {
          if constexpr (decltype(order)::value == 1 || decltype(noise)::value == 0) f(rows, order, noise, mask);
        });
      });
    });
  });
}

}  // namespace
}  // namespace mixdq
