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

/* InstructPix2Pix (mixdq_sampler_step3): three UNet rows per image -- e_t with text and image, e_i with the image only,
 * e_u with neither -- and two scales, diffusers' expression in its own left-to-right order:
 *   e = (e_u + g * (e_t - e_i)) + gi * (e_i - e_u)      six roundings: two differences, two products, two sums
 * With e_i == e_u the second product is +-0 and e is the two-row guidance of (e_u, e_t), as a value. */
MIXDQ_HD float mixdq_sampler_guided_eps3(float e_t, float e_i, float e_u, float g, float gi) {
  return MIXDQ_ADD_RN(MIXDQ_ADD_RN(e_u, MIXDQ_MUL_RN(g, MIXDQ_SUB_RN(e_t, e_i))),
                      MIXDQ_MUL_RN(gi, MIXDQ_SUB_RN(e_i, e_u)));
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

/* ---- Gaussian noise (mixdq_randn_f32, mixdq_sampler_step[_masked]_rng, csrc/sampler.hip), same rule: integers, and
 * FP32 with every rounding explicit.  A counter-based generator: nothing is kept between calls, any element can be
 * computed alone, and the value of an element depends on (seed, element, step, stream) only.
 *
 * Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants):
 * ten rounds of  (c0, c1, c2, c3) <- (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)),  the key
 * bumped by (W0, W1) between rounds. */
#define MIXDQ_PHILOX_M0 0xD2511F53u
#define MIXDQ_PHILOX_M1 0xCD9E8D57u
#define MIXDQ_PHILOX_W0 0x9E3779B9u
#define MIXDQ_PHILOX_W1 0xBB67AE85u

MIXDQ_HD void mixdq_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)MIXDQ_PHILOX_M0 * c0, p1 = (uint64_t)MIXDQ_PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += MIXDQ_PHILOX_W0; k1 += MIXDQ_PHILOX_W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

/* The correctly rounded square root: the compiler's own under -fno-fast-math (on the device clang expands it to the
 * correctly rounded sequence; HIP's __fsqrt_rn is, without OCML_BASIC_ROUNDED_OPERATIONS, the 1-ulp native one). */
#define MIXDQ_SQRT_RN(a) __builtin_sqrtf(a)

/* log(k * 2^-24) for k = 1 .. 2^24, max error 0.851 ulp over all 2^24 arguments (measured against float64; 0 at
 * k = 2^24 exactly, never positive).  k is exact as a float; its exponent is split off in integers so that the
 * mantissa m lies in [2/3, 4/3), then log1p(m - 1) by a degree-11 polynomial in two interleaved chains and
 * e * ln 2 added with one fma.  Minimax coefficients as published by N. Juffa for single-precision logf. */
MIXDQ_HD float mixdq_rng_log_u24(uint32_t k) {
  const float x = (float)k;
  uint32_t bits;
  memcpy(&bits, &x, 4);
  const uint32_t e = (bits - 0x3F2AAAABu) & 0xFF800000u;
  float m = mixdq_bits_to_float(bits - e);
  const float i = (float)(((int32_t)e >> 23) - 24);
  m = m - 1.0f;
  const float s = m * m;
  float r = -0.130310059f, t = 0.140869141f;
  r = __builtin_fmaf(r, s, -0.121483512f);
  t = __builtin_fmaf(t, s, 0.139814854f);
  r = __builtin_fmaf(r, s, -0.166846126f);
  t = __builtin_fmaf(t, s, 0.200120345f);
  r = __builtin_fmaf(r, s, -0.249996200f);
  r = __builtin_fmaf(t, m, r);
  r = __builtin_fmaf(r, m, 0.333331972f);
  r = __builtin_fmaf(r, m, -0.5f);
  r = __builtin_fmaf(r, s, m);
  return __builtin_fmaf(i, 0.693147182f, r);
}

/* sin and cos of 2 pi j 2^-24 for j = 0 .. 2^24 - 1, each max error 1.015 ulp over all 2^24 arguments (measured against
 * float64; exact zeros where the functions have them).  The reduction is in integers and exact: the top three bits are
 * the octant, the low 21 (in odd octants their complement to 2^21) the place inside it, x = r * 2^-21 in [0, 1], angle
 * x * pi/4.  sin(x pi/4) = x * (pi/4 + y * S(y)) and cos(x pi/4) = 1 + y * C(y) with y = x * x, S and C of degree 2
 * and 3 (Chebyshev-node fits, 3.4e-9 and 2.7e-10 relative before rounding); pi/4 enters as an FP32 high part and a
 * correction so that the leading term is rounded once. */
MIXDQ_HD void mixdq_rng_sincos_u24(uint32_t j, float* sn, float* cs) {
  const uint32_t octant = j >> 21;
  uint32_t r = j & 0x1FFFFFu;
  if (octant & 1u) r = 0x200000u - r;
  const float x = (float)r * 4.76837158203125e-07f;            /* 2^-21: exact */
  const float y = x * x;
  float q = __builtin_fmaf(-3.595429006963968e-05f, y, 0.0024900068528950214f);
  q = __builtin_fmaf(q, y, -0.08074543625116348f);
  const float w = __builtin_fmaf(q, y, -2.4276526e-08f);
  const float xw = x * w;
  const float s = __builtin_fmaf(x, mixdq_bits_to_float(0x3F490FDBu), xw);
  float p = __builtin_fmaf(3.541952764862799e-06f, y, -0.00032596138771623373f);
  p = __builtin_fmaf(p, y, 0.01585433818399906f);
  p = __builtin_fmaf(p, y, -0.3084251284599304f);
  const float c = __builtin_fmaf(p, y, 1.0f);
  const int swap = ((octant + 1u) >> 1) & 1u;                  /* octants 1, 2, 5, 6 */
  float so = swap ? c : s, co = swap ? s : c;
  if (octant >= 4u) so = -so;
  if (((octant + 2u) >> 2) & 1u) co = -co;                     /* octants 2 .. 5 */
  *sn = so;
  *cs = co;
}

/* Two 32-bit words to two standard normals (Box-Muller on 24-bit uniforms): u1 = ((ra >> 8) + 1) 2^-24 in (0, 1],
 * u2 = (rb >> 8) 2^-24 in [0, 1), rad = sqrt(-2 log u1) (the doubling exact, the root correctly rounded), z0 = rad *
 * cos(2 pi u2), z1 = rad * sin(2 pi u2).  |z| <= sqrt(48 ln 2) ~ 5.77: the distribution has no longer tail. */
MIXDQ_HD void mixdq_rng_box_muller(uint32_t ra, uint32_t rb, float* z0, float* z1) {
  const float rad = MIXDQ_SQRT_RN(MIXDQ_MUL_RN(-2.0f, mixdq_rng_log_u24((ra >> 8) + 1u)));
  float sn, cs;
  mixdq_rng_sincos_u24(rb >> 8, &sn, &cs);
  *z0 = MIXDQ_MUL_RN(rad, cs);
  *z1 = MIXDQ_MUL_RN(rad, sn);
}

/* The four outputs of one Philox call as four normals: (r0, r1) -> (z0, z1), (r2, r3) -> (z2, z3). */
MIXDQ_HD void mixdq_rng_normals4(const uint32_t r[4], float z[4]) {
  mixdq_rng_box_muller(r[0], r[1], &z[0], &z[1]);
  mixdq_rng_box_muller(r[2], r[3], &z[2], &z[3]);
}

/* Which call produces which element.  Image b of a batch has a 64-bit seed; element e of that image, counted in
 * storage (NHWC) order, is lane e & 3 of the call with key (lo32(seed), hi32(seed)) and counter (lo32(e >> 2),
 * hi32(e >> 2), step, stream) -- stream: what the noise is for (MIXDQ_RNG_STREAM_*, mixdq_hip.h), step: the absolute
 * index of the sampler step that consumes it (0 for the other streams).  mixdq_rng_quad: elements 4 * quad .. + 3. */
MIXDQ_HD void mixdq_rng_bits(uint64_t seed, uint64_t quad, uint32_t step, uint32_t stream, uint32_t r[4]) {
  const uint32_t ctr[4] = {(uint32_t)quad, (uint32_t)(quad >> 32), step, stream};
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  mixdq_philox4x32_10(ctr, key, r);
}

MIXDQ_HD void mixdq_rng_quad(uint64_t seed, uint64_t quad, uint32_t step, uint32_t stream, float z[4]) {
  uint32_t r[4];
  mixdq_rng_bits(seed, quad, step, stream, r);
  mixdq_rng_normals4(r, z);
}

/* One element alone: the same call, the Box-Muller pair of its lane only -- the same bits as mixdq_rng_quad's. */
MIXDQ_HD float mixdq_rng_normal_at(uint64_t seed, uint64_t e, uint32_t step, uint32_t stream) {
  uint32_t r[4];
  float z0, z1;
  mixdq_rng_bits(seed, e >> 2, step, stream, r);
  if (e & 2u) mixdq_rng_box_muller(r[2], r[3], &z0, &z1);
  else mixdq_rng_box_muller(r[0], r[1], &z0, &z1);
  return (e & 1u) ? z1 : z0;
}

/* ---- separable resampling (mixdq_resample, mixdq_resample_paste_u8, csrc/image.hip).  One output value is two
 * chains of explicit fused multiply-adds over host-made FP32 weight tables, each starting at +0: for every source row
 * of its vertical window the horizontal chain over taps i = 0 .. Tx-1 in order (an FP32 value, never rounded to 8
 * bits), then the vertical chain of those values over j = 0 .. Ty-1 in order.  A tap whose weight is zero (either
 * sign) is SKIPPED, not multiplied: the zero padding of a shorter table row never meets a NaN or inf of a float
 * source.  Source elements enter as (float)u for uint8 (pixel scale 0 .. 255), as their value for FP16 / FP32, and in
 * MASK mode as 255.0f where the element is set by mixdq_mask_to_latent's rule and 0.0f elsewhere. */
MIXDQ_HD float mixdq_resample_tap(float acc, float w, float v) {
  return (w == 0.0f) ? acc : __builtin_fmaf(w, v, acc);
}

/* An accumulator on the pixel scale as a byte: NaN and everything <= 0 is 0, everything >= 255 is 255, between them
 * rintf (half to even). */
MIXDQ_HD uint8_t mixdq_round_u8(float a) {
  if (a != a) return 0;
  if (a <= 0.0f) return 0;
  if (a >= 255.0f) return 255;
  return (uint8_t)(int)__builtin_rintf(a);
}

/* The feathered paste, in integers: (m*d + (255-m)*o + 127) / 255 -- the nearest integer to the exact quotient
 * (255 is odd: the remainder is never half of it, no tie exists).  m = 0 gives o, m = 255 gives d. */
MIXDQ_HD uint8_t mixdq_blend_u8(uint8_t m, uint8_t d, uint8_t o) {
  const uint32_t s = (uint32_t)m * d + (uint32_t)(255u - m) * o + 127u;
  return (uint8_t)(s / 255u);
}

/* ---- guidance rescale (mixdq_sampler_step_rescaled, csrc/sampler_rescale.hip), same rule: Lin et al., "Common
 * diffusion noise schedules and sample steps are flawed", diffusers' rescale_noise_cfg.  Per image, over all of its
 * n_image storage elements, with t the text-conditioned model output (two rows: row block 1; three rows: block 0, e_t;
 * FP16 read exactly as FP32) and e the guided output (mixdq_sampler_guided_eps / _eps3 of the same elements):
 *   s  = sqrt(M2_t / M2_e)          M2 = sum((v - mean)^2): the n - 1 of an unbiased std cancels in the quotient
 *   r  = 1 + phi * (s - 1)          diffusers' phi * s + (1 - phi), written so that s == 1 gives r == 1 exactly
 *   e' = e * r                      one product (mixdq_sampler_rescaled); the rest of the step is unchanged
 * r = 1 where M2_e == 0, M2_t == 0 or n_image == 1 (OUR definition: diffusers divides by zero there and returns NaN).
 *
 * M2 is NOT E[x^2] - mean^2 (which cancels: a latent with mean 64 and unit spread loses four digits in FP32).  The image
 * is cut into CHUNKS of MIXDQ_RESCALE_CHUNK = 2048 consecutive elements (256 lanes x 8; the last chunk holds the
 * remaining count >= 1 elements, any number).  Per chunk and tensor, two passes over the same values:
 *   mean_c = S(v) / (float)count                 the division correctly rounded
 *   M2_c   = S((v - mean_c) * (v - mean_c))      one difference and one product per element, each rounded
 * where S is a sum of 2048 terms in a FIXED order, elements beyond `count` entering as +0:
 *   lane l (0 .. 255):  p_l = ((((((v[8l] + v[8l+1]) + v[8l+2]) + ... ) + v[8l+7])       seven sums in storage order
 *   wave w (lanes 64w .. 64w + 63): for k = 1, 2, 4, 8, 16, 32 in turn every lane replaces p_l by p_l + p_(l ^ k) --
 *                        a balanced pairwise tree; after the six rounds all 64 lanes hold the wave's sum W_w
 *   S = ((W_0 + W_1) + W_2) + W_3                three sums
 * mixdq_rescale_lane_sum is the first line; the other two are adds a caller arranges (csrc/sampler_rescale.hip,
 * tests/rescale_ref.py).  The chunks of an image are then combined IN CHUNK ORDER by Chan's update, starting from
 * (n, mean, M2) = (0, 0, 0) -- mixdq_rescale_combine, every operation one rounding, the integers converted to FP32 by
 * round-to-nearest:
 *   tot = n + k                                  integers (k: the chunk's count)
 *   d   = mean_c - mean
 *   mean' = mean + d * ((float)k / (float)tot)                                    division, product, sum
 *   M2'   = M2 + (M2_c + (d * d) * (((float)n * (float)k) / (float)tot))          product, product, division, product, two sums
 * The first chunk gives (mean_0, M2_0) exactly: k / k == 1 and n == 0.  The division is the language's own (IEEE,
 * correctly rounded: hipcc's default for gfx950 as for the host), the square root MIXDQ_SQRT_RN: no hardware estimate
 * enters, so a device and a host compiler agree bit for bit. */
#define MIXDQ_RESCALE_CHUNK 2048
#define MIXDQ_DIV_RN(a, b) ((a) / (b))

MIXDQ_HD float mixdq_rescale_lane_sum(const float v[8]) {
  float s = MIXDQ_ADD_RN(v[0], v[1]);
  for (int j = 2; j < 8; ++j) s = MIXDQ_ADD_RN(s, v[j]);
  return s;
}

/* One element's term of the second pass. */
MIXDQ_HD float mixdq_rescale_sqdev(float v, float mean_c) {
  const float d = MIXDQ_SUB_RN(v, mean_c);
  return MIXDQ_MUL_RN(d, d);
}

MIXDQ_HD void mixdq_rescale_combine(int64_t n, int64_t k, float mean_c, float m2_c, float* mean, float* m2) {
  const float fn = (float)n, fk = (float)k, ft = (float)(n + k);
  const float d = MIXDQ_SUB_RN(mean_c, *mean);
  *mean = MIXDQ_ADD_RN(*mean, MIXDQ_MUL_RN(d, MIXDQ_DIV_RN(fk, ft)));
  const float q = MIXDQ_DIV_RN(MIXDQ_MUL_RN(fn, fk), ft);
  *m2 = MIXDQ_ADD_RN(*m2, MIXDQ_ADD_RN(m2_c, MIXDQ_MUL_RN(MIXDQ_MUL_RN(d, d), q)));
}

MIXDQ_HD float mixdq_rescale_factor(float m2_t, float m2_e, float phi, int64_t n_image) {
  if (m2_e == 0.0f || m2_t == 0.0f || n_image == 1) return 1.0f;
  const float s = MIXDQ_SQRT_RN(MIXDQ_DIV_RN(m2_t, m2_e));
  return MIXDQ_ADD_RN(1.0f, MIXDQ_MUL_RN(phi, MIXDQ_SUB_RN(s, 1.0f)));
}

MIXDQ_HD float mixdq_sampler_rescaled(float e, float r) { return MIXDQ_MUL_RN(e, r); }

/* ---- ControlNet residuals (mixdq_control_add_f16, csrc/control.hip), same rule: diffusers' arithmetic on FP16 tensors,
 * every operation one FP32 rounding of exact FP16 operands followed by the FP16 rounding the caller applies
 * (f32_to_f16_rn on the device, a cast on the host).  For one element, skip s, the residuals r_k of nets k = 0 .. K-1 in
 * order, and their FP32 scales c_k of this step:
 *   t_k = f16_rn(f32(r_k) * c_k)                 ControlNetModel: sample * conditioning_scale
 *   acc = t_first;  acc = f16_rn(f32(acc) + f32(t_k)) for each later net        MultiControlNetModel, left to right
 *   out = f16_rn(f32(s) + f32(acc))              the UNet's skip + residual
 * A net whose c_k == 0 (either sign) is SKIPPED, its residual not read (diffusers multiplies by 0: the two differ for a
 * non-finite r_k and in the sign of a zero); with every net skipped out is s's own bits.  mixdq_control_scaled and
 * mixdq_control_sum are the two FP32 operations. */
MIXDQ_HD float mixdq_control_scaled(float r, float c) { return MIXDQ_MUL_RN(r, c); }

MIXDQ_HD float mixdq_control_sum(float a, float b) { return MIXDQ_ADD_RN(a, b); }

/* ---- ControlNet hint ingest (mixdq_hint_to_nhwc8_f16, csrc/control.hip): a uint8 pixel on the [0, 1] scale, the FP32
 * value whose FP16 rounding the conditioning embedding reads: f32(u) / 255.0f, the division correctly rounded -- what
 * image.float() / 255 computes. */
MIXDQ_HD float mixdq_hint_unit(uint32_t u) { return MIXDQ_DIV_RN((float)u, 255.0f); }

#endif /* MIXDQ_MATH_H_ */
