// Decoupled cross-attention for gfx950 (IP-Adapter) at SD 1.5's head widths 40, 80 and 160, ONE launch:
//   out = attn(q, K_text, V_text) + s_0 * attn(q, K_ip0, V_ip0) + s_1 * attn(q, K_ip1, V_ip1) + ...
// The sibling of attn_ip_kernel (csrc/attention_ip.hip, head width 64) on the geometry of attn_hd_short_kernel
// (csrc/attention.hip; AttnHd<D> in csrc/attn_core.h).  No reference counterpart.  Arithmetic: include/mixdq_math.h
// (mixdq_ip_scaled / mixdq_ip_sum): every term is mixdq_attention_f16's FP16 result at that width, bit for bit, the sum
// diffusers' half-tensor arithmetic, left to right.  DESIGN.md section 3.38.
//   work split   128 query rows per workgroup, 32 per wave; the KS Q^T fragments stay in registers for every key set.
//   loads        everything is issued up front behind one s_waitcnt vmcnt(0) and one barrier.  Text K / V: the short
//                kernel's 64-key stage images (pitches PK / PV, no swizzle, the same slot map), one per 64 text keys.
//                Image K / V behind them in 32-KEY blocks: 32 K rows at pitch PK, then 32 V rows at pitch PV -- half a
//                stage image, so the K reads and the ds_read_b64_tr_b16 V reads are the short kernel's with another
//                base.  A block is staged as one run of 16-B slots in whole 1-KB LDS-DMA groups (every lane of a group
//                writes), so its pitch is half a stage rounded up to 1 KB: 9 / 12 / 21 KB at D = 40 / 80 / 160; the
//                slots past the V rows receive a copy of the block's first chunk.  An adapter's keys are padded to
//                whole blocks; a skipped adapter (s_j == 0, a scalar: wave-uniform) issues no staging loads.
//   text pass    the short kernel's sequence; then O is normalised and rounded to FP16 -- the running FP16 result.
//   image pass   the o / lsum accumulators are reused for each adapter in turn, 64 keys (two blocks) per softmax step;
//                only REAL blocks are multiplied (an all-absent block is P = 0: +0 into every accumulator, the signed
//                zero of an FP32 underflow aside: mixdq_math.h), then acc = f16(acc + f16(o_j * s_j)).
//   the result   D = 40 / 80: packed in 10 / 20 registers, in the lane layout of the output staging, written to the
//                staging rows after the barrier that ends the K / V reads.  D = 160: the short kernel's 214 registers
//                leave no room for 40 more, so the barrier moves behind the TEXT pass, the text result is written to
//                the wave's staging rows over the dead text images, and each adapter's term is added there (a lane
//                reads and writes its own 8 bytes: no synchronisation); the image blocks start behind the staging.
//   epilogue     the short kernel's: whole output rows from the staging, FP16 or through to_out.0's quantizer.
#include "attn_ip.h"

namespace mixdq {
namespace {

constexpr int kMaxLds = 160 * 1024;                  // a CU's LDS: the most one workgroup can have

template <int D>
struct IpHd {
  using G = AttnHd<D>;
  static constexpr bool PARK = D > 80;               // the running FP16 result lives in the staging rows, not registers
  // Waves per SIMD the register budget is compiled for.  The short kernel's 4 and 3 at D = 40 and 80 do not hold the
  // packed result (hipcc spills 4 and 2 registers to scratch; profiles/ip_adapter_hd_isa.txt), and the LDS of a
  // 77-key launch with one block (43 / 58 KB of the CU's 160 KB) admits no more than 3 and 2 workgroups anyway.
  static constexpr int WPE = D <= 40 ? 3 : 2;
  static constexpr int STAGING = 4 * 32 * G::PO;
  static constexpr int KSLOTS = kBlockKeys * G::PCK;                 // 16-B slots of a block: the K rows ...
  static constexpr int SLOTS = kBlockKeys * (G::PCK + G::PCV);       // ... and all of it
  static constexpr int GROUPS = (SLOTS + 63) / 64;                   // 1-KB LDS-DMA groups of a block
  static constexpr int BLOCK = GROUPS * 1024;
  // the image blocks start behind the text stages AND the output staging (which D = 160 writes while they are read)
  static constexpr int img0(int ntiles) { return ntiles * G::SB > STAGING ? ntiles * G::SB : STAGING; }
  static constexpr int smem(int ntiles, int blocks) { return img0(ntiles) + blocks * BLOCK; }
};

// One softmax step of one wave over up to 64 keys = two 32-key halves in LDS: attn_hd_short_kernel's loop body with the
// addresses as arguments.  koff / voff: byte offsets of the K and V rows of the two halves; nblk (wave-uniform): halves
// that hold a real key; nreal: real keys of the step (absent ones are masked to -inf).
template <int D>
__device__ __forceinline__ void ip_hd_softmax_step(v16f (&o)[AttnHd<D>::DB], v16f& lsum, float& m_i,
                                                   const v8h (&qf)[AttnHd<D>::KS], const v8h& ones, float c, unsigned k_a,
                                                   unsigned v_a, const unsigned (&koff)[2], const unsigned (&voff)[2],
                                                   int nblk, int nreal, int hh) {
  using G = AttnHd<D>;
  const v8h zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  v16f sc[2];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
    for (int i = 0; i < 16; ++i) sc[kb][i] = 0.f;
    if (kb < nblk) {
      v8h kf[G::KS];
      static_for<0, G::KS>([&](auto ksc) {
        constexpr int ks = decltype(ksc)::value;
        lds_read128_imm<ks * 32>(kf[ks], k_a + koff[kb]);
      });
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int ks = 0; ks < G::KS; ++ks) asm volatile("" : "+v"(kf[ks]));
      if constexpr (D % 16 != 0) kf[G::KS - 1] = hh ? zero8 : kf[G::KS - 1];   // d D .. KS * 16 - 1: zeros
#pragma unroll
      for (int ks = 0; ks < G::KS; ++ks)
        sc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ks], qf[ks], sc[kb], 0, 0, 0);
    }
  }
  if (nreal < kKeys) {                               // mask the absent keys (a whole absent half included)
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
    for (int i = 0; i < 16; ++i) {
#pragma unroll
      for (int db = 0; db < G::DB; ++db) o[db][i] *= alpha;
    }
    lsum[0] *= alpha;
  }
  m_i = m_new;
  // O^T += V^T P^T, 16 keys at a time (the short kernel's order)
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    if (kb >= nblk) break;
    static_for<0, 2>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      VFrag vf[G::DB];
      static_for<0, G::DB>([&](auto dbc) {
        constexpr int db = decltype(dbc)::value;
        tr_read2_at<16 * u * G::PV + 64 * db, (16 * u + 8) * G::PV + 64 * db>(vf[db], v_a + voff[kb]);
      });
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int db = 0; db < G::DB; ++db) asm volatile("" : "+v"(vf[db].h));
#pragma unroll
      for (int db = 0; db < G::DB; ++db)
        o[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[db].h, pf[kb][u], o[db], 0, 0, 0);
      lsum = __builtin_amdgcn_mfma_f32_32x32x16_f16(ones, pf[kb][u], lsum, 0, 0, 0);
    });
  }
}

// A4: the output quantizer is a 4-bit one (MIXDQ_FLAG_A4_0; common.h quantize_pack8<., true>).
template <int D, bool QUANT, bool A4 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(IpHd<D>::WPE, IpHd<D>::WPE)))
void attn_ip_hd_kernel(const AttnIpParams p) {
  using G = AttnHd<D>;
  using I = IpHd<D>;
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
  constexpr int WAVES = 4;
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
  const unsigned img0 = (unsigned)I::img0(ntiles);
  const v8h zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  // Q^T fragments: lane's query row, d = 16 ks + 8 h .. + 7 (zeros past D)
  v8h qf[G::KS];
  {
    const int qr = min(q0 + l32, p.tq - 1);
    const __half* qrow = p.q + b * p.q_bs + (long)qr * p.q_rs + head * D + hh * 8;
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks)
      qf[ks] = 16 * ks + 8 * hh < D ? *reinterpret_cast<const v8h*>(qrow + ks * 16) : zero8;
  }
  // text staging: as attn_hd_short_kernel (same images, same slot map), tile t in stage t
  {
    const char* kbase = reinterpret_cast<const char*>(p.k + b * p.k_bs + head * D);
    const char* vbase = reinterpret_cast<const char*>(p.v + b * p.v_bs + head * D);
    const unsigned krs = 2u * (unsigned)p.k_rs, vrs = 2u * (unsigned)p.v_rs;
    for (int t = 0; t < ntiles; ++t) {
      char* dst = smem + t * G::SB;
      for (int i = wave; i < G::PCK + G::PCV; i += WAVES) {   // wave-uniform
        const bool isv = i >= G::PCK;
        const int pc = isv ? G::PCV : G::PCK;
        const int s = (isv ? i - G::PCK : i) * 64 + lane;
        const int row = s / pc;
        int ch = s - row * pc;
        if (ch >= G::DC) ch = 0;                          // pitch padding: a copy of the row's first chunk
        const unsigned key = (unsigned)min(t * kKeys + row, p.tkv - 1);
        glds16((isv ? vbase : kbase) + (key * (isv ? vrs : krs) + (unsigned)ch * 16), dst + i * 1024);
      }
    }
  }
  // image staging: a block is one run of SLOTS 16-B slots (K rows, V rows) in GROUPS 1-KB groups dealt over the waves
#pragma unroll
  for (int j = 0; j < kMaxIp; ++j) {
    if (j >= p.n_ip || s_ip[j] == 0.f) continue;     // (wave-uniform: scalars) a skipped adapter issues none
    const long boff = b * p.ip_bs[j] + head * D;
    const char* kbase = reinterpret_cast<const char*>(p.ip_k[j] + boff);
    const char* vbase = reinterpret_cast<const char*>(p.ip_v[j] + boff);
    const unsigned srs = p.ip_rs2[j];
    const int last_key = p.ip_tok[j] - 1;
    for (int g = blk0[j]; g < blk0[j + 1]; ++g) {
      char* dst = smem + img0 + g * I::BLOCK;
      for (int i = wave; i < I::GROUPS; i += WAVES) {
        int s = i * 64 + lane;
        if (s >= I::SLOTS) s = 0;                    // behind the V rows: a copy of the block's first chunk
        const bool isv = s >= I::KSLOTS;
        const int pc = isv ? G::PCV : G::PCK;
        if (isv) s -= I::KSLOTS;
        const int row = s / pc;
        int ch = s - row * pc;
        if (ch >= G::DC) ch = 0;
        const unsigned key = (unsigned)min((g - blk0[j]) * kBlockKeys + row, last_key);
        glds16((isv ? vbase : kbase) + (key * srs + (unsigned)ch * 16), dst + i * 1024);
      }
    }
  }
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  const int q4 = (lane & 15) >> 2, pp = lane & 3, g16 = (lane >> 4) & 1;
  const unsigned k_a = lds0 + l32 * G::PK + hh * 16;                         // row l32, chunk 2 ks + h
  const unsigned v_a = lds0 + (4 * hh + q4) * G::PV + 32 * g16 + 8 * pp;     // (relative to a V image)
  v16f o[G::DB], lsum;
  float m_i;
  auto reset = [&]() {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
#pragma unroll
      for (int db = 0; db < G::DB; ++db) o[db][i] = 0.f;
      lsum[i] = 0.f;
    }
    m_i = -INFINITY;
  };
  reset();
  const float c = p.scale_log2;
  v8h ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (_Float16)1.f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- text keys: attn_hd_short_kernel's sequence ----
  for (int t = 0; t < ntiles; ++t) {
    const unsigned koff[2] = {(unsigned)(t * G::SB), (unsigned)(t * G::SB + 32 * G::PK)};
    const unsigned voff[2] = {(unsigned)(t * G::SB + kKeys * G::PK), (unsigned)(t * G::SB + kKeys * G::PK + 32 * G::PV)};
    ip_hd_softmax_step<D>(o, lsum, m_i, qf, ones, c, k_a, v_a, koff, voff, 2, min(p.tkv - t * kKeys, kKeys), hh);
  }
  // The running FP16 result, [db][g] = columns 32 db + 8 g + 4 hh + 0..3 of the lane's query row: registers, or the
  // lane's 8 bytes of the wave's staging rows.  fold(s): acc = the normalised o (the text term; s unused) or
  // acc = f16(acc + f16(normalised o * s)).
  char* Os = smem + wave * (32 * G::PO);
  v4h acc[G::DB][4];
  auto fold = [&](auto first, float s) {
    const float inv = 1.f / lsum[0];
#pragma unroll
    for (int db = 0; db < G::DB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (32 * db + 8 * g >= D) continue;            // (compile-time) columns past the head
        v4h* slot = reinterpret_cast<v4h*>(Os + l32 * G::PO + (32 * db + 8 * g + 4 * hh) * 2);
        v4h w;
        if constexpr (!decltype(first)::value) w = I::PARK ? *slot : acc[db][g];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const _Float16 oj = normalised_f16(o[db][4 * g + e], inv, e);
          if constexpr (decltype(first)::value) {
            w[e] = oj;
          } else {
            const _Float16 t = f16_rn(mixdq_ip_scaled((float)oj, s));
            w[e] = f16_rn(mixdq_ip_sum((float)w[e], (float)t));
          }
        }
        if constexpr (I::PARK) *slot = w;
        else acc[db][g] = w;
      }
  };
  if constexpr (I::PARK) __syncthreads();            // every wave is done with the text images: the staging may overlay
  fold(std::true_type{}, 0.f);
  // ---- image keys, one adapter at a time on the same accumulators ----
  for (int j = 0; j < p.n_ip; ++j) {
    const float s = j == 0 ? s_ip[0] : j == 1 ? s_ip[1] : j == 2 ? s_ip[2] : s_ip[3];
    if (s == 0.f) continue;                          // (wave-uniform: a scalar)
    const int g0 = j == 0 ? blk0[0] : j == 1 ? blk0[1] : j == 2 ? blk0[2] : blk0[3];
    const int g1 = j == 0 ? blk0[1] : j == 1 ? blk0[2] : j == 2 ? blk0[3] : blk0[4];
    const int tok = j == 0 ? p.ip_tok[0] : j == 1 ? p.ip_tok[1] : j == 2 ? p.ip_tok[2] : p.ip_tok[3];
    reset();
    for (int g = g0; g < g1; g += 2) {
      const unsigned koff[2] = {img0 + g * I::BLOCK, img0 + (g + 1) * I::BLOCK};
      const unsigned voff[2] = {koff[0] + kBlockKeys * G::PK, koff[1] + kBlockKeys * G::PK};
      ip_hd_softmax_step<D>(o, lsum, m_i, qf, ones, c, k_a, v_a, koff, voff, min(g1 - g, 2),
                            min(tok - (g - g0) * kBlockKeys, kKeys), hh);
    }
    fold(std::false_type{}, s);
  }
  if constexpr (!I::PARK) {
    __syncthreads();                                 // every wave is done with the K / V images
#pragma unroll
    for (int db = 0; db < G::DB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (32 * db + 8 * g < D)
          *reinterpret_cast<v4h*>(Os + l32 * G::PO + (32 * db + 8 * g + 4 * hh) * 2) = acc[db][g];
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // wave-private staging: no block barrier
  constexpr int NCH = 32 * G::DC;                     // 16-B chunks of the wave's 32 output rows
#pragma unroll
  for (int i = 0; i < (NCH + 63) / 64; ++i) {
    const int id = lane + 64 * i, row = id / G::DC, ch = id - row * G::DC;
    if (id >= NCH || q0 + row >= p.tq) continue;
    const uint4 w = *reinterpret_cast<const uint4*>(Os + row * G::PO + ch * 16);
    const long off = b * p.o_bs + (long)(q0 + row) * p.o_rs + head * D + ch * 8;
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

template <int D>
bool ip_hd_fits(int tkv, int blocks) {
  return IpHd<D>::smem((tkv + kKeys - 1) / kKeys, blocks) <= kMaxLds;
}

// The shapes the kernel takes (include/mixdq_hip.h); everything a caller can ask without pointers.
int ip_hd_shape_status(int head_dim, int tkv, int n_ip, const int* ip_tokens) {
  if (n_ip < 1 || n_ip > kMaxIp || !ip_tokens) return MIXDQ_ERR_INVALID_ARG;
  if ((head_dim != 40 && head_dim != 80 && head_dim != 160) || tkv < 1 || tkv > 2 * kKeys) return MIXDQ_ERR_SHAPE;
  for (int j = 0; j < n_ip; ++j)
    if (ip_tokens[j] < 1 || ip_tokens[j] > 2 * kKeys) return MIXDQ_ERR_SHAPE;
  const int blocks = ip_blocks(n_ip, ip_tokens);
  if (blocks > kMaxIpBlocks) return MIXDQ_ERR_SHAPE;
  const bool fits = head_dim == 40 ? ip_hd_fits<40>(tkv, blocks) : head_dim == 80 ? ip_hd_fits<80>(tkv, blocks)
                                                                                  : ip_hd_fits<160>(tkv, blocks);
  return fits ? MIXDQ_OK : MIXDQ_ERR_SHAPE;
}

template <int D>
int launch_attn_ip_hd(const AttnIpParams& p, int batch, int blocks, bool quant, bool a4, hipStream_t stream) {
  const int grid = p.qblocks * p.heads * batch;
  const int smem = IpHd<D>::smem((p.tkv + kKeys - 1) / kKeys, blocks);
  int status = MIXDQ_OK;
  with_bool(quant, [&](auto qq) {
    with_bool(a4, [&](auto a) {
      constexpr bool Q = decltype(qq)::value, A4 = decltype(a)::value;
      if constexpr (Q || !A4) {                          // A4 is a form of the output quantizer
        status = lds_opt_in<&attn_ip_hd_kernel<D, Q, A4>>(kMaxLds);   // (whatever this launch stages)
        if (status != MIXDQ_OK) return;
        hipLaunchKernelGGL((attn_ip_hd_kernel<D, Q, A4>), dim3(grid), dim3(256), smem, stream, p);
      }
    });
  });
  return status != MIXDQ_OK ? status : launch_status();
}

}  // namespace
}  // namespace mixdq

using namespace mixdq;

extern "C" int mixdq_attention_f16_ip_hd_supported(int head_dim, int tkv, int n_ip, const int* ip_tokens) {
  return ip_hd_shape_status(head_dim, tkv, n_ip, ip_tokens) == MIXDQ_OK ? 1 : 0;
}

extern "C" int mixdq_attention_f16_ip_hd(const void* q, const void* k, const void* v, void* out,
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
  const int st = ip_prepare(p, quant, a4, ip_hd_shape_status, q, k, v, out, batch, heads, head_dim, tq, tkv,
                            q_batch_stride, q_row_stride, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride,
                            out_batch_stride, out_row_stride, n_ip, ip_k, ip_v, ip_tokens, ip_batch_stride,
                            ip_row_stride, ip_scale, softmax_scale, out_scale_inv, out_zero_point, flags);
  if (st != MIXDQ_OK || p.qblocks == 0) return st;
  const int blocks = ip_blocks(n_ip, ip_tokens);
  return head_dim == 40   ? launch_attn_ip_hd<40>(p, batch, blocks, quant, a4, stream)
         : head_dim == 80 ? launch_attn_ip_hd<80>(p, batch, blocks, quant, a4, stream)
                          : launch_attn_ip_hd<160>(p, batch, blocks, quant, a4, stream);
}
