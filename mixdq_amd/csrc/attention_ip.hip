// Decoupled cross-attention for gfx950 (IP-Adapter; diffusers' IPAdapterAttnProcessor2_0), head_dim 64, ONE launch:
//   out = attn(q, K_text, V_text) + s_0 * attn(q, K_ip0, V_ip0) + s_1 * attn(q, K_ip1, V_ip1) + ...
// with up to four small image key sets, each with a softmax of its own, and to_out.0's quantizer in the epilogue.  No
// reference counterpart.  Arithmetic: include/mixdq_math.h (mixdq_ip_scaled / mixdq_ip_sum): every term is
// mixdq_attention_f16's FP16 result, bit for bit, the sum diffusers' half-tensor arithmetic, left to right.
//
// A sibling of attn_short_kernel (csrc/attention.hip) -- a cross-attention workgroup's life is one memory round trip
// and a microsecond of arithmetic, and this kernel keeps it at ONE round trip with the image keys added:
//   work split   128 query rows per workgroup, 32 per wave; the Q^T fragments stay in registers for every key set.
//   loads        everything is issued up front: the text K / V into the two 64-key stage images of the short kernel
//                (32 KB), the image K / V behind them in 32-KEY blocks (K 4 KB | V 4 KB each; an adapter's keys are
//                padded to whole blocks, at most four blocks per launch: dynamic LDS = 32 KB + 8 KB per block).  One
//                s_waitcnt vmcnt(0), one barrier.  A block is a half of the short kernel's tile image with the same
//                swizzle, so the K reads and the transposed V reads are the short kernel's with another base.
//   scales       s_j are scalar loads at entry, like the quantizer's scalars: one captured graph serves every scale.
//                s_j == 0 skips adapter j wave-uniformly: no staging loads, no arithmetic.
//   text pass    the short kernel's sequence; then O is normalised, rounded to FP16 and kept PACKED in 16 registers,
//                in the lane layout of the output staging.
//   image pass   the o / lsum accumulators are reused for each adapter in turn, 64 keys (two blocks) per softmax step
//                as the short kernel groups them -- but only REAL blocks are multiplied: the second block of a step
//                that has no real key is all -inf scores, P = 0, and adds +0 to every accumulator, so leaving its
//                MFMAs out changes no bit (except the sign of a zero that FP32 underflow produced: mixdq_math.h).
//   epilogue     acc = f16(acc + f16(o_j * s_j)) in registers, then the short kernel's staging, store and quantizer.
#include "attn_ip.h"

namespace mixdq {
namespace {

constexpr int kBlockBytes = 2 * kBlockKeys * kRow;   // K rows then V rows, 128 B each
constexpr int kTextBytes = 2 * kStageBytes;          // the short kernel's two K | V stage images

// One softmax step of one wave over up to 64 keys = two 32-key blocks in LDS: attn_short_kernel's loop body, with the
// block addresses as arguments.  koff / voff: byte offsets of the K and V rows of the two blocks; nblk (wave-uniform):
// blocks that hold a real key; nreal: real keys of the step (absent ones are masked to -inf).
__device__ __forceinline__ void ip_softmax_step(v16f (&o)[2], v16f& lsum, float& m_i, const v8h (&qf)[4], const v8h& ones,
                                                float c, const unsigned (&k_a)[4], unsigned v_a0, unsigned v_a1,
                                                const unsigned (&koff)[2], const unsigned (&voff)[2], int nblk,
                                                int nreal, int hh) {
  v16f sc[2];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
    for (int i = 0; i < 16; ++i) sc[kb][i] = 0.f;
    if (kb < nblk) {
      v8h kf[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        kf[ks] = *(const __attribute__((address_space(3))) v8h*)(size_t)(k_a[ks] + koff[kb]);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        sc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ks], qf[ks], sc[kb], 0, 0, 0);
    }
  }
  if (nreal < kKeys) {                               // mask the absent keys (a whole absent block included)
    const int lim = nreal - 4 * hh;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (32 * kb + 8 * (r >> 2) + (r & 3) >= lim) sc[kb][r] = -INFINITY;
  }
  float mx = sc[0][0];
#pragma unroll
  for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sc[0][r]);
#pragma unroll
  for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[1][r]);
  mx = half_max(mx);
  const float m_new = fmaxf(m_i, mx);
  const bool grew = m_new > m_i;
  const float mc = m_new * c;
  v8h pf[2][2];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      pf[kb][r >> 3][r & 7] = (_Float16)__builtin_amdgcn_exp2f(__builtin_fmaf(sc[kb][r], c, -mc));
  if (__builtin_amdgcn_ballot_w64(grew)) {
    const float alpha = __builtin_amdgcn_exp2f((m_i - m_new) * c);
#pragma unroll
    for (int i = 0; i < 16; ++i) { o[0][i] *= alpha; o[1][i] *= alpha; }
    lsum[0] *= alpha;
  }
  m_i = m_new;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    if (kb >= nblk) break;
    VFrag vf[2][2];
    const unsigned a0 = v_a0 + voff[kb], a1 = v_a1 + voff[kb];
    tr_read2_imm<0 * kRow>(vf[0][0], a0);
    tr_read2_imm<0 * kRow>(vf[0][1], a1);
    tr_read2_imm<16 * kRow>(vf[1][0], a0);
    tr_read2_imm<16 * kRow>(vf[1][1], a1);
    s_waitcnt_lgkm0();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int db = 0; db < 2; ++db)
        o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[u][db].h, pf[kb][u], o[db], 0, 0, 0);
      lsum = __builtin_amdgcn_mfma_f32_32x32x16_f16(ones, pf[kb][u], lsum, 0, 0, 0);
    }
  }
}

// Three waves per SIMD (three workgroups per CU): the short kernel's 128 registers plus the 16 of the packed text result
// do not fit four (hipcc then spills 24 registers to scratch; profiles/ip_adapter_isa.txt).
// A4: the output quantizer is a 4-bit one (MIXDQ_FLAG_A4_0; common.h quantize_pack8<., true>).
template <bool QUANT, bool A4 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void attn_ip_kernel(const AttnIpParams p) {
  MIXDQ_ARGS_NOW(p.q, p.k, p.v, p.out, p.q_bs, p.q_rs, p.k_bs, p.k_rs, p.v_bs, p.v_rs, p.o_bs, p.o_rs,
                 p.tq, p.tkv, p.heads, p.qblocks);
  MIXDQ_ARGS_NOW(p.scale_log2, p.s_inv, p.zp, p.unfused, p.n_ip, p.ip_scale);
  float s_inv = 0.f, zp = 0.f;                       // scalar loads at entry
  if constexpr (QUANT) {
    s_inv = scalar_load(p.s_inv);
    zp = scalar_load(p.zp);
  }
  float s_ip[kMaxIp];
  int blk0[kMaxIp + 1];                              // first block of adapter j in the image area
  blk0[0] = 0;
#pragma unroll
  for (int j = 0; j < kMaxIp; ++j) {
    s_ip[j] = j < p.n_ip ? scalar_load(p.ip_scale + j) : 0.f;
    blk0[j + 1] = blk0[j] + (j < p.n_ip ? (p.ip_tok[j] + kBlockKeys - 1) / kBlockKeys : 0);
  }
  constexpr int WAVES = 4, NI = 16 / WAVES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, hh = lane >> 5;
  const int blk = blockIdx.x;                        // (no XCD map: a head's K / V are a few KB, every L2 may hold them)
  const int qb = blk % p.qblocks;
  const int head = (blk / p.qblocks) % p.heads;
  const int b = blk / (p.qblocks * p.heads);
  const int q0 = qb * (WAVES * 32) + wave * 32;
  const int ntiles = (p.tkv + kKeys - 1) / kKeys;      // 1 or 2

  v8h qf[4];
  {
    const int qr = min(q0 + l32, p.tq - 1);
    const __half* qrow = p.q + b * p.q_bs + (long)qr * p.q_rs + head * kHeadDim + hh * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const v8h*>(qrow + ks * 16);
  }
  const int srow = lane >> 3, spos = lane & 7;
  // text staging: as attn_short_kernel (waves 0, 1: K, waves 2, 3: V; same images), real tiles only
  {
    const bool stage_v = wave * NI >= 8;
    const char* sbase = reinterpret_cast<const char*>(
        (stage_v ? p.v + b * p.v_bs : p.k + b * p.k_bs) + head * kHeadDim);
    const unsigned srs = 2u * (unsigned)(stage_v ? p.v_rs : p.k_rs);
    const int last_key = p.tkv - 1;
    for (int t = 0; t < ntiles; ++t) {
      char* dst = smem + t * kStageBytes + wave * NI * 1024;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int krow = ((wave * NI + i) & 7) * 8 + srow;
        const int sw = stage_v ? ((krow >> 1) & 1) << 2 : (krow >> 1) & 7;
        const int key = min(t * kKeys + krow, last_key);   // past the end: the last key, masked below
        glds16(sbase + ((unsigned)key * srs + (unsigned)((spos ^ sw) * 16)), dst + i * 1024);
      }
    }
  }
  // image staging: a block is eight 1-KB row groups (K 0..3, V 4..7), two per wave; a skipped adapter issues none
  {
    const bool stage_v = wave >= 2;
#pragma unroll
    for (int j = 0; j < kMaxIp; ++j) {
      if (j >= p.n_ip || s_ip[j] == 0.f) continue;
      const char* sbase = reinterpret_cast<const char*>((stage_v ? p.ip_v[j] : p.ip_k[j]) + b * p.ip_bs[j] + head * kHeadDim);
      const unsigned srs = p.ip_rs2[j];
      const int last_key = p.ip_tok[j] - 1;
      for (int g = blk0[j]; g < blk0[j + 1]; ++g) {
        char* dst = smem + kTextBytes + g * kBlockBytes + wave * 2048;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int krow = ((wave * 2 + i) & 3) * 8 + srow;
          const int sw = stage_v ? ((krow >> 1) & 1) << 2 : (krow >> 1) & 7;
          const int key = min((g - blk0[j]) * kBlockKeys + krow, last_key);
          glds16(sbase + ((unsigned)key * srs + (unsigned)((spos ^ sw) * 16)), dst + i * 1024);
        }
      }
    }
  }
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  unsigned k_a[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) k_a[ks] = lds0 + l32 * kRow + (((2 * ks + hh) ^ ((l32 >> 1) & 7)) << 4);
  const int q4 = (lane & 15) >> 2, pp = lane & 3, g16 = (lane >> 4) & 1;
  const int v_rd0 = (4 * hh + q4) * kRow + (((2 * g16 + (pp >> 1)) ^ (((q4 >> 1) & 1) << 2)) << 4) + 8 * (pp & 1);
  const unsigned v_a0 = lds0 + v_rd0, v_a1 = lds0 + (v_rd0 ^ 64);
  v16f o[2], lsum;
#pragma unroll
  for (int i = 0; i < 16; ++i) { o[0][i] = 0.f; o[1][i] = 0.f; lsum[i] = 0.f; }
  float m_i = -INFINITY;
  const float c = p.scale_log2;
  v8h ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (_Float16)1.f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- text keys: attn_short_kernel's sequence ----
  for (int t = 0; t < ntiles; ++t) {
    const unsigned koff[2] = {(unsigned)(t * kStageBytes), (unsigned)(t * kStageBytes + 32 * kRow)};
    const unsigned voff[2] = {koff[0] + kTileBytes, koff[1] + kTileBytes};
    ip_softmax_step(o, lsum, m_i, qf, ones, c, k_a, v_a0, v_a1, koff, voff, 2, min(p.tkv - t * kKeys, kKeys), hh);
  }
  v4h acc[2][4];                                     // the FP16 result, packed: [db][g] = columns 32 db + 8 g + 4 hh + 0..3
  {
    const float inv = 1.f / lsum[0];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[db][g][e] = normalised_f16(o[db][4 * g + e], inv, e);
  }
  // ---- image keys, one adapter at a time on the same accumulators ----
  for (int j = 0; j < p.n_ip; ++j) {
    const float s = j == 0 ? s_ip[0] : j == 1 ? s_ip[1] : j == 2 ? s_ip[2] : s_ip[3];
    if (s == 0.f) continue;                          // (wave-uniform: a scalar)
    const int g0 = j == 0 ? blk0[0] : j == 1 ? blk0[1] : j == 2 ? blk0[2] : blk0[3];
    const int g1 = j == 0 ? blk0[1] : j == 1 ? blk0[2] : j == 2 ? blk0[3] : blk0[4];
    const int tok = j == 0 ? p.ip_tok[0] : j == 1 ? p.ip_tok[1] : j == 2 ? p.ip_tok[2] : p.ip_tok[3];
#pragma unroll
    for (int i = 0; i < 16; ++i) { o[0][i] = 0.f; o[1][i] = 0.f; lsum[i] = 0.f; }
    m_i = -INFINITY;
    for (int g = g0; g < g1; g += 2) {
      const unsigned koff[2] = {(unsigned)(kTextBytes + g * kBlockBytes), (unsigned)(kTextBytes + (g + 1) * kBlockBytes)};
      const unsigned voff[2] = {koff[0] + kBlockKeys * kRow, koff[1] + kBlockKeys * kRow};
      ip_softmax_step(o, lsum, m_i, qf, ones, c, k_a, v_a0, v_a1, koff, voff, min(g1 - g, 2),
                      min(tok - (g - g0) * kBlockKeys, kKeys), hh);
    }
    const float inv = 1.f / lsum[0];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const _Float16 oj = normalised_f16(o[db][4 * g + e], inv, e);
          const _Float16 t = f16_rn(mixdq_ip_scaled((float)oj, s));
          acc[db][g][e] = f16_rn(mixdq_ip_sum((float)acc[db][g][e], (float)t));
        }
  }
  __syncthreads();                                   // every wave is done with the K / V images
  char* Os = smem + wave * (32 * kORow);
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<v4h*>(Os + l32 * kORow + (32 * db + 8 * g + 4 * hh) * 2) = acc[db][g];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // wave-private staging: no block barrier
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = lane + 64 * i, row = id >> 3, ch = id & 7;
    if (q0 + row >= p.tq) continue;
    const uint4 w = *reinterpret_cast<const uint4*>(Os + row * kORow + ch * 16);
    const long off = b * p.o_bs + (long)(q0 + row) * p.o_rs + head * kHeadDim + ch * 8;
    if constexpr (!QUANT) {
      *reinterpret_cast<uint4*>(reinterpret_cast<__half*>(p.out) + off) = w;
    } else {
      const __half* hv = reinterpret_cast<const __half*>(&w);
      float x[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = __half2float(hv[e]);
      *reinterpret_cast<uint2*>(reinterpret_cast<int8_t*>(p.out) + off) =
          p.unfused ? quantize_pack8<true, A4>(x, s_inv, zp) : quantize_pack8<false, A4>(x, s_inv, zp);
    }
  }
}

// The shapes the kernel takes (include/mixdq_hip.h); everything a caller can ask without pointers.
int ip_shape_status(int head_dim, int tkv, int n_ip, const int* ip_tokens) {
  if (n_ip < 1 || n_ip > kMaxIp || !ip_tokens) return MIXDQ_ERR_INVALID_ARG;
  if (head_dim != kHeadDim || tkv < 1 || tkv > 2 * kKeys) return MIXDQ_ERR_SHAPE;
  int blocks = 0;
  for (int j = 0; j < n_ip; ++j) {
    if (ip_tokens[j] < 1 || ip_tokens[j] > 2 * kKeys) return MIXDQ_ERR_SHAPE;
    blocks += (ip_tokens[j] + kBlockKeys - 1) / kBlockKeys;
  }
  return blocks <= kMaxIpBlocks ? MIXDQ_OK : MIXDQ_ERR_SHAPE;
}

}  // namespace
}  // namespace mixdq

using namespace mixdq;

extern "C" int mixdq_attention_f16_ip_supported(int head_dim, int tkv, int n_ip, const int* ip_tokens) {
  return ip_shape_status(head_dim, tkv, n_ip, ip_tokens) == MIXDQ_OK ? 1 : 0;
}

extern "C" int mixdq_attention_f16_ip(const void* q, const void* k, const void* v, void* out,
                                      int batch, int heads, int head_dim, int tq, int tkv,
                                      int64_t q_batch_stride, int64_t q_row_stride,
                                      int64_t k_batch_stride, int64_t k_row_stride,
                                      int64_t v_batch_stride, int64_t v_row_stride,
                                      int64_t out_batch_stride, int64_t out_row_stride,
                                      int n_ip, const void* const* ip_k, const void* const* ip_v,
                                      const int* ip_tokens, const int64_t* ip_batch_stride,
                                      const int64_t* ip_row_stride, const float* ip_scale,
                                      float softmax_scale, const float* out_scale_inv,
                                      const float* out_zero_point, int flags, mixdq_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  AttnIpParams p;
  bool quant = false, a4 = false;
  const int st = ip_prepare(p, quant, a4, ip_shape_status, q, k, v, out, batch, heads, head_dim, tq, tkv, q_batch_stride,
                            q_row_stride, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride, out_batch_stride,
                            out_row_stride, n_ip, ip_k, ip_v, ip_tokens, ip_batch_stride, ip_row_stride, ip_scale,
                            softmax_scale, out_scale_inv, out_zero_point, flags);
  if (st != MIXDQ_OK || p.qblocks == 0) return st;
  const int blocks = ip_blocks(n_ip, ip_tokens);
  const int grid = p.qblocks * heads * batch;
  const int smem = kTextBytes + blocks * kBlockBytes;   // the output staging overlays the text images
  with_bool(quant, [&](auto qq) {
    with_bool(a4, [&](auto a) {
      constexpr bool Q = decltype(qq)::value, A4 = decltype(a)::value;
      if constexpr (Q || !A4)                            // A4 is a form of the output quantizer
        hipLaunchKernelGGL((attn_ip_kernel<Q, A4>), dim3(grid), dim3(256), smem, stream, p);
    });
  });
  return launch_status();
}
