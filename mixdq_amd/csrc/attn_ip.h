// What the two decoupled cross-attention units share (csrc/attention_ip.hip: head width 64; csrc/attention_ip_hd.hip:
// head widths 40 / 80 / 160): the kernel arguments, the scalar-load and rounding helpers, and the C-ABI entry's argument
// checks (include/mixdq_hip.h: one argument list, one set of status codes).  gfx950 only.
#pragma once
#include "common.h"
#include "attn_core.h"
#include "../../include/mixdq_math.h"

namespace mixdq {
namespace {

constexpr int kMaxIp = MIXDQ_IP_MAX_ADAPTERS;
constexpr int kMaxIpBlocks = MIXDQ_IP_MAX_BLOCKS;
constexpr int kBlockKeys = 32;                       // an image key block: K rows, then V rows

struct AttnIpParams {
  const __half* q; const __half* k; const __half* v;
  void* out;                                         // f16 rows or int8 rows
  long q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs;   // batch / row strides in elements
  int tq, tkv, heads, qblocks;
  int unfused, n_ip;
  float scale_log2;                                  // softmax scale * log2(e)
  const float* s_inv; const float* zp;
  const float* ip_scale;                             // device, [n_ip]
  const __half* ip_k[kMaxIp]; const __half* ip_v[kMaxIp];
  long ip_bs[kMaxIp];
  unsigned ip_rs2[kMaxIp];                           // row stride in BYTES
  int ip_tok[kMaxIp];
};
static_assert(sizeof(AttnIpParams) < 512, "the operands travel in the kernel arguments");

// (as csrc/attention.hip: the 16-byte LDS-DMA)
__device__ __forceinline__ void glds16(const void* gsrc, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)gsrc,
      (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
__device__ __forceinline__ float scalar_load(const float* p) {
  return *(const __attribute__((address_space(4))) float*)p;
}
// FP32 -> FP16 with the FP32 value made opaque first (common.h f32_to_f16_rn, as a _Float16)
__device__ __forceinline__ _Float16 f16_rn(float v) {
  asm("" : "+v"(v));
  return (_Float16)v;
}
// The normalised output o * inv as FP16, element e (0..3) of a group of four accumulator registers, with the roundings
// attn_short_kernel's and attn_hd_short_kernel's `(_Float16)(o[..] * inv)` HAVE in the library: hipcc compiles that loop
// to v_fma_mixlo_f16 for elements 0 and 3 of every group (the exact product rounded ONCE to FP16) and to a FP32 multiply
// followed by a conversion for elements 1 and 2 (rounded to FP32, then to FP16), at every head width (DESIGN.md sections
// 3.37, 3.38).  The two differ in about one result in 2^13, and every term of these kernels is specified as that kernel's
// bits, so the choice is written out here instead of left to the compiler; tests/test_attention_ip_gpu.py and
// tests/test_attention_ip_hd_gpu.py hold the kernels together.
__device__ __forceinline__ _Float16 normalised_f16(float o, float inv, int e) {
  if (e == 0 || e == 3) {
    unsigned d = 0;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "+v"(d) : "v"(inv), "v"(o));
    return __builtin_bit_cast(_Float16, (unsigned short)d);
  }
  return f16_rn(__fmul_rn(o, inv));
}

// The argument checks of mixdq_attention_f16_ip / mixdq_attention_f16_ip_hd, in the order that decides which status a
// call with several faults gets, and the kernel arguments filled in.  shape_status: the unit's own shape predicate.
// Returns a status; MIXDQ_OK with p.qblocks == 0: nothing to write, launch nothing.
inline int ip_prepare(AttnIpParams& p, bool& quant, bool& a4, int (*shape_status)(int, int, int, const int*),
                      const void* q, const void* k, const void* v, void* out, int batch, int heads, int head_dim, int tq,
                      int tkv, int64_t q_batch_stride, int64_t q_row_stride, int64_t k_batch_stride, int64_t k_row_stride,
                      int64_t v_batch_stride, int64_t v_row_stride, int64_t out_batch_stride, int64_t out_row_stride,
                      int n_ip, const void* const* ip_k, const void* const* ip_v, const int* ip_tokens,
                      const int64_t* ip_batch_stride, const int64_t* ip_row_stride, const float* ip_scale,
                      float softmax_scale, const float* out_scale_inv, const float* out_zero_point, int flags) {
  p.qblocks = 0;
  if (batch < 0 || heads <= 0 || tq < 0) return MIXDQ_ERR_INVALID_ARG;
  if ((out_scale_inv == nullptr) != (out_zero_point == nullptr)) return MIXDQ_ERR_INVALID_ARG;
  if (const int st = shape_status(head_dim, tkv, n_ip, ip_tokens)) return st;
  if (!ip_k || !ip_v || !ip_batch_stride || !ip_row_stride || !ip_scale) return MIXDQ_ERR_INVALID_ARG;
  if (flags & MIXDQ_FLAG_ACT_ANY) return MIXDQ_ERR_UNSUPPORTED;
  if (flags & (MIXDQ_FLAG_CAUSAL | 0xff00)) return MIXDQ_ERR_SHAPE;      // one launch form, no mask
  if (flags & (MIXDQ_FLAG_A4_1 | MIXDQ_FLAG_A4_2)) return MIXDQ_ERR_UNSUPPORTED;   // one quantizer: slot 0
  if (batch == 0 || tq == 0) return MIXDQ_OK;       // nothing to write (pointers may be null)
  if (!q || !k || !v || !out) return MIXDQ_ERR_INVALID_ARG;
  quant = out_scale_inv != nullptr;
  a4 = quant && (flags & MIXDQ_FLAG_A4_0);
  // 16-byte vector accesses: rows of 8 halfs, bases and strides multiples of 8 elements
  const int64_t strides[] = {q_batch_stride, q_row_stride, k_batch_stride, k_row_stride,
                             v_batch_stride, v_row_stride, out_batch_stride, out_row_stride};
  for (int64_t s : strides)
    if (s % 8) return MIXDQ_ERR_ALIGNMENT;
  // key-row offsets are formed in 32 bits
  if ((int64_t)tkv * k_row_stride >= (1ll << 31) || (int64_t)tkv * v_row_stride >= (1ll << 31))
    return MIXDQ_ERR_SHAPE;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) return MIXDQ_ERR_ALIGNMENT;
  if ((uintptr_t)out & (quant ? 7 : 15)) return MIXDQ_ERR_ALIGNMENT;
  if ((uintptr_t)ip_scale & 3) return MIXDQ_ERR_ALIGNMENT;

  p.q = (const __half*)q; p.k = (const __half*)k; p.v = (const __half*)v; p.out = out;
  p.q_bs = q_batch_stride; p.q_rs = q_row_stride;
  p.k_bs = k_batch_stride; p.k_rs = k_row_stride;
  p.v_bs = v_batch_stride; p.v_rs = v_row_stride;
  p.o_bs = out_batch_stride; p.o_rs = out_row_stride;
  p.tq = tq; p.tkv = tkv; p.heads = heads;
  p.scale_log2 = softmax_scale * 1.4426950408889634f;
  p.s_inv = out_scale_inv; p.zp = out_zero_point;
  p.unfused = (flags & MIXDQ_FLAG_UNFUSED) ? 1 : 0;
  p.n_ip = n_ip; p.ip_scale = ip_scale;
  for (int j = 0; j < kMaxIp; ++j) {
    const bool on = j < n_ip;
    if (on) {
      if (!ip_k[j] || !ip_v[j]) return MIXDQ_ERR_INVALID_ARG;
      if (ip_batch_stride[j] % 8 || ip_row_stride[j] % 8 || (((uintptr_t)ip_k[j] | (uintptr_t)ip_v[j]) & 15))
        return MIXDQ_ERR_ALIGNMENT;
      if (ip_row_stride[j] < 0 || (int64_t)ip_tokens[j] * ip_row_stride[j] >= (1ll << 31)) return MIXDQ_ERR_SHAPE;
    }
    p.ip_k[j] = on ? (const __half*)ip_k[j] : nullptr;
    p.ip_v[j] = on ? (const __half*)ip_v[j] : nullptr;
    p.ip_bs[j] = on ? ip_batch_stride[j] : 0;
    p.ip_rs2[j] = on ? 2u * (unsigned)ip_row_stride[j] : 0u;
    p.ip_tok[j] = on ? ip_tokens[j] : 0;
  }
  if ((long)((tq + 127) / 128) * heads * batch > 0x7fffffffl) return MIXDQ_ERR_INVALID_ARG;
  p.qblocks = (tq + 127) / 128;
  return MIXDQ_OK;
}
inline int ip_blocks(int n_ip, const int* ip_tokens) {
  int blocks = 0;
  for (int j = 0; j < n_ip; ++j) blocks += (ip_tokens[j] + kBlockKeys - 1) / kBlockKeys;
  return blocks;
}

}  // namespace
}  // namespace mixdq
