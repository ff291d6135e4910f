// Shared pieces of the FP16 attention core (csrc/attention.hip) that the fused
// to_q + cross-attention epilogue of csrc/igemm.hip and the decoupled cross-attention units (csrc/attn_ip.h) reuse:
// tile geometry, LDS image layout, the transposed-read helpers and the geometry of head widths 40 / 80 / 160.
// gfx950 only.
#pragma once
#include "common.h"

namespace mixdq {
namespace {

constexpr int kHeadDim = 64;
constexpr int kKeys = 64;            // keys per tile
constexpr int kRow = 128;            // K and V images: 64 halfs per key, XOR-swizzled 16-B chunks
constexpr int kTileBytes = kKeys * kRow;          // one K (or V) tile
constexpr int kStageBytes = 2 * kTileBytes;       // K tile then V tile
constexpr int kORow = 144;           // output staging row (32 x 144 B per wave)

__device__ __forceinline__ float half_max(float x) {
  // max over lanes l and l^32
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

typedef int v2i __attribute__((ext_vector_type(2)));
union VFrag { struct { v2i lo, hi; } r; v8h h; };

// Two transposed reads (keys k..k+3 and k+8..k+11 of 16 output columns) = one A operand.
template <int OFF>
__device__ __forceinline__ void tr_read2_imm(VFrag& f, unsigned addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%3\n\tds_read_b64_tr_b16 %1, %2 offset:%4"
               : "=&v"(f.r.lo), "=&v"(f.r.hi)
               : "v"(addr), "n"(OFF), "n"(OFF + 8 * kRow)
               : "memory");
}
__device__ __forceinline__ void s_waitcnt_lgkm0() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);   // keep register-only MFMAs behind the wait
}

template <int OFF>
__device__ __forceinline__ void lds_read128_imm(v8h& d, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory");
}

// ---- head widths 40, 80, 160: the geometry of attn_hd_kernel / attn_hd_short_kernel (csrc/attention.hip, where the
// layouts are described) and of the decoupled cross-attention at those widths (csrc/attention_ip_hd.hip) ----
template <int D>
struct AttnHd {
  static constexpr int DC = D / 8;                                   // 16-B chunks of a head row
  static constexpr int KS = (D + 15) / 16;
  static constexpr int DB = (D + 31) / 32;
  static constexpr int PCK = DC | 1;
  static constexpr int PCV = DC <= 4 ? 4 : 4 + 8 * ((DC - 4 + 7) / 8);
  static constexpr int PK = 16 * PCK, PV = 16 * PCV;
  static constexpr int SB = kKeys * (PK + PV);                       // one stage: K image then V image
  static constexpr int PO = DB * 64 + 16;                            // output staging row
  static constexpr int smem(int waves) { return 2 * SB > waves * 32 * PO ? 2 * SB : waves * 32 * PO; }
  // the short-key form: waves per SIMD its register budget is compiled for (D = 160 keeps O^T alone in 80 registers)
  static constexpr int SHORT_WPE = D <= 40 ? 4 : D <= 80 ? 3 : 2;
  static constexpr int smem_short(int ntiles) { return ntiles * SB > 4 * 32 * PO ? ntiles * SB : 4 * 32 * PO; }
  static_assert(D % 8 == 0 && DB * 64 <= PV && 2 * D <= PK, "geometry");
};

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

template <int OFF0, int OFF1>
__device__ __forceinline__ void tr_read2_at(VFrag& f, unsigned addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%3\n\tds_read_b64_tr_b16 %1, %2 offset:%4"
               : "=&v"(f.r.lo), "=&v"(f.r.hi)
               : "v"(addr), "n"(OFF0), "n"(OFF1)
               : "memory");
}

}  // namespace
}  // namespace mixdq
