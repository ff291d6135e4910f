/*
 * mixdq_math.h -- the arithmetic SPECIFICATION of the transcendental steps used by the fused
 * producer kernels (SiLU, GELU), written so that a host C compiler and hipcc produce bit-identical
 * results: only IEEE-754 binary32 +, -, *, /, fmaf, rintf and integer bit operations, every fused
 * multiply-add explicit (compile with -ffp-contract=off), no libm transcendental, no fast-math.
 *
 * The reference computes SiLU / GELU with stock PyTorch FP16 ops; those are
 * accurate to ~1 ulp of FP32 before rounding to FP16, as are these, so results agree with PyTorch to
 * within one FP16 ulp (tests state the tolerance).  Between the HIP kernels and the CPU oracle the
 * agreement is exact by construction, which is what lets the fused kernels be tested bit-for-bit.
 */
#ifndef MIXDQ_MATH_H_
#define MIXDQ_MATH_H_

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MIXDQ_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define MIXDQ_HD static inline
#endif

MIXDQ_HD float mixdq_bits_to_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

/* exp(x), |rel err| < 2 ulp.  Cephes-style: n = rint(x*log2(e)), r = x - n*ln2 (two-term),
 * degree-5 polynomial, scale by 2^n through the exponent bits.  Results below 2^-126 flush to 0,
 * above FLT_MAX give +inf. */
MIXDQ_HD float mixdq_expf(float x) {
  if (x != x) return x;
  if (x > 88.72283f) return mixdq_bits_to_float(0x7f800000u);
  if (x < -87.33654f) return 0.0f;
  const float n = __builtin_rintf(x * 1.44269504088896341f);
  float r = __builtin_fmaf(n, -0.693359375f, x);
  r = __builtin_fmaf(n, 2.12194440e-4f, r);
  float p = 1.9875691500e-4f;
  p = __builtin_fmaf(p, r, 1.3981999507e-3f);
  p = __builtin_fmaf(p, r, 8.3334519073e-3f);
  p = __builtin_fmaf(p, r, 4.1665795894e-2f);
  p = __builtin_fmaf(p, r, 1.6666665459e-1f);
  p = __builtin_fmaf(p, r, 5.0000001201e-1f);
  p = __builtin_fmaf(p * r, r, r) + 1.0f;
  int e = (int)n;            /* -126 .. 128 */
  float scale;
  if (e > 127) {             /* split the scale so 2^128 never has to be formed */
    p = p * 2.0f;
    e -= 1;
  }
  scale = mixdq_bits_to_float((uint32_t)(e + 127) << 23);
  return p * scale;
}

/* SiLU on an FP32 value: x / (1 + exp(-x)) with a correctly rounded division. */
MIXDQ_HD float mixdq_siluf(float x) { return x / (1.0f + mixdq_expf(-x)); }

/* erf(x), max error 1.5 ulp (|abs err| < 7e-8), two branches, one exp, no division:
 *   |x| <  0.921875 : x + x * P(x^2)                      (degree-5 polynomial in x^2)
 *   |x| >= 0.921875 : +-(1 - exp(-|x| + |x| * Q(|x|)))     (degree-6 polynomial, mixed x / x^2)
 * Minimax coefficients as published by N. Juffa for single-precision erff. */
MIXDQ_HD float mixdq_erff(float a) {
  uint32_t ua;
  memcpy(&ua, &a, 4);
  const float t = mixdq_bits_to_float(ua & 0x7fffffffu);   /* |a| */
  const float s = a * a;
  float r;
  if (t >= 0.921875f) {
    float u;
    r = __builtin_fmaf(-1.72853470e-5f, t, 3.83197126e-4f);
    u = __builtin_fmaf(-3.88396438e-3f, t, 2.42546219e-2f);
    r = __builtin_fmaf(r, s, u);
    r = __builtin_fmaf(r, t, -1.06777877e-1f);
    r = __builtin_fmaf(r, t, -6.34846687e-1f);
    r = __builtin_fmaf(r, t, -1.28717512e-1f);
    r = __builtin_fmaf(r, t, -t);
    r = 1.0f - mixdq_expf(r);
    uint32_t ur;
    memcpy(&ur, &r, 4);
    r = mixdq_bits_to_float((ur & 0x7fffffffu) | (ua & 0x80000000u));   /* copysign(r, a) */
  } else {                     /* also taken by NaN: propagates */
    r = -5.96761703e-4f;
    r = __builtin_fmaf(r, s, 4.99119423e-3f);
    r = __builtin_fmaf(r, s, -2.67681349e-2f);
    r = __builtin_fmaf(r, s, 1.12819925e-1f);
    r = __builtin_fmaf(r, s, -3.76125336e-1f);
    r = __builtin_fmaf(r, s, 1.28379166e-1f);
    r = __builtin_fmaf(r, a, a);
  }
  return r;
}

/* GELU (erf form, torch's default): 0.5 * x * (1 + erf(x / sqrt(2))). */
MIXDQ_HD float mixdq_geluf(float x) {
  return 0.5f * x * (1.0f + mixdq_erff(x * 0.70710678118654752440f));
}

/* quick-GELU (CLIP ViT-L's activation): x * sigmoid(1.702 x) as x / (1 + exp(-(1.702 x))) -- the product rounded,
 * negated, one exp, the sum rounded, a correctly rounded division. */
MIXDQ_HD float mixdq_quick_geluf(float x) { return x / (1.0f + mixdq_expf(-(1.702f * x))); }

/* ---- sampler step (mixdq_sampler_step, csrc/sampler.hip): classifier-free guidance + the affine scheduler
 * update.  Every operation is one IEEE binary32 round-to-nearest +, - or *, never contracted: on the device the
 * _rn intrinsics (which the compiler may not fuse), on a host compiler plain operators under -ffp-contract=off.
 *   e  = eps_u + g * (eps_c - eps_u)            three roundings: difference, product, sum
 *   x' = (a*x + b*e) + c*n                      each product rounded, then the two sums; without noise a*x + b*e
 *   in = f16_rn(x' * s_next)                    the product rounded to FP32 first, then to FP16 by the caller */
#if defined(__HIP_DEVICE_COMPILE__)
#define MIXDQ_MUL_RN(a, b) __fmul_rn((a), (b))
#define MIXDQ_ADD_RN(a, b) __fadd_rn((a), (b))
#define MIXDQ_SUB_RN(a, b) __fsub_rn((a), (b))
#else
#define MIXDQ_MUL_RN(a, b) ((a) * (b))
#define MIXDQ_ADD_RN(a, b) ((a) + (b))
#define MIXDQ_SUB_RN(a, b) ((a) - (b))
#endif

MIXDQ_HD float mixdq_sampler_guided_eps(float eps_u, float eps_c, float g) {
  return MIXDQ_ADD_RN(eps_u, MIXDQ_MUL_RN(g, MIXDQ_SUB_RN(eps_c, eps_u)));
}

MIXDQ_HD float mixdq_sampler_update(float x, float e, float a, float b) {
  return MIXDQ_ADD_RN(MIXDQ_MUL_RN(a, x), MIXDQ_MUL_RN(b, e));
}

MIXDQ_HD float mixdq_sampler_update_noise(float x, float e, float n, float a, float b, float c) {
  return MIXDQ_ADD_RN(mixdq_sampler_update(x, e, a, b), MIXDQ_MUL_RN(c, n));
}

/* The FP32 value whose FP16 rounding is the UNet's next input. */
MIXDQ_HD float mixdq_sampler_scaled_input(float x_next, float s_next) { return MIXDQ_MUL_RN(x_next, s_next); }

/* ---- inpainting (mixdq_sampler_step_masked, csrc/sampler.hip), same rule.  After the scheduler update the region the
 * mask keeps is overwritten with the image latents z noised to the NEXT step's level with the run's initial noise n0
 * (diffusers' inpainting with a 4-channel UNet); m = 1 repaints, m = 0 keeps, values between blend:
 *   k   = (p*z) + (q*n0)                        two products and a sum; (p, q) = blend[*step]
 *   x'' = ((1 - m) * k) + (m * x')              one difference, two products and a sum
 * For m == 0 the result is k and for m == 1 it is x' (finite operands; up to the sign of zero: -0 + +0 is +0). */
MIXDQ_HD float mixdq_sampler_blend(float x_new, float z, float n0, float m, float p, float q) {
  const float k = MIXDQ_ADD_RN(MIXDQ_MUL_RN(p, z), MIXDQ_MUL_RN(q, n0));
  return MIXDQ_ADD_RN(MIXDQ_MUL_RN(MIXDQ_SUB_RN(1.0f, m), k), MIXDQ_MUL_RN(m, x_new));
}

/* ---- multistep sampler step (mixdq_sampler_step_2m, csrc/sampler.hip), same rule.  DPM-Solver++ 2M works on the
 * data prediction x0 and keeps the previous step's one as its history h:
 *   x0 = (u*x) + (v*e)                          two products and a sum; e the guided epsilon
 *   x' = ((A*x) + (B*x0)) + (D*h)               second-order step: each product rounded, then the two sums
 * The first-order step is mixdq_sampler_update(x, x0, A, B1): h is not an operand of it. */
MIXDQ_HD float mixdq_sampler_x0(float x, float e, float u, float v) {
  return MIXDQ_ADD_RN(MIXDQ_MUL_RN(u, x), MIXDQ_MUL_RN(v, e));
}

MIXDQ_HD float mixdq_sampler_update_2m(float x, float x0, float h, float A, float B, float D) {
  return MIXDQ_ADD_RN(MIXDQ_ADD_RN(MIXDQ_MUL_RN(A, x), MIXDQ_MUL_RN(B, x0)), MIXDQ_MUL_RN(D, h));
}

/* ---- VAE decoder end (mixdq_composite_u8, csrc/vae.hip): one FP16 image value (given as its exact FP32 value) as
 * the pixel vae.to_uint8 makes of it, ((f32(v) / 2 + 0.5).clamp(0, 1) * 255).round() with round-half-even:
 * the halving is exact, then one sum, the clamp, one product, rintf -- each one FP32 operation.  -inf is 0, +inf
 * 255.  NaN is 0: the torch expression carries the NaN to its conversion to uint8, which on the GPU goes through a
 * 64-bit integer whose conversion from NaN is 0. */
MIXDQ_HD uint8_t mixdq_to_uint8(float v) {
  if (v != v) return 0;
  float t = MIXDQ_ADD_RN(MIXDQ_MUL_RN(v, 0.5f), 0.5f);
  t = __builtin_fminf(__builtin_fmaxf(t, 0.0f), 1.0f);
  return (uint8_t)(int)__builtin_rintf(MIXDQ_MUL_RN(t, 255.0f));
}

/* ---- VAE encoder ends (csrc/vae.hip), same rule: one rounding per operation, never contracted.
 * The posterior sample of an AutoencoderKL (DiagonalGaussianDistribution: logvar clamped to [-30, 20]), times the
 * scaling factor:  z = (mean + exp(0.5 * logvar) * n) * sf;  without noise the mode, mean * sf. */
MIXDQ_HD float mixdq_vae_latent(float mean, float logvar, float n, float sf) {
  const float lv = __builtin_fminf(__builtin_fmaxf(logvar, -30.0f), 20.0f);
  const float std = mixdq_expf(MIXDQ_MUL_RN(0.5f, lv));
  return MIXDQ_MUL_RN(MIXDQ_ADD_RN(mean, MIXDQ_MUL_RN(std, n)), sf);
}

MIXDQ_HD float mixdq_vae_latent_mode(float mean, float sf) { return MIXDQ_MUL_RN(mean, sf); }

/* A uint8 pixel as the FP32 value whose FP16 rounding the encoder reads: u * (2/255) - 1, the constant 2/255 rounded
 * to FP32 (0x3C008081).  For all 256 values its FP16 rounding is that of u / 127.5 - 1 computed exactly. */
MIXDQ_HD float mixdq_pixel_to_unit(uint32_t u) {
  return MIXDQ_SUB_RN(MIXDQ_MUL_RN((float)u, mixdq_bits_to_float(0x3C008081u)), 1.0f);
}

#endif /* MIXDQ_MATH_H_ */
