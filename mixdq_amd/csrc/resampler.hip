// The two launches a perceiver Resampler (IP-Adapter "plus") needs and the other kernels cannot give
// (include/mixdq_hip.h mixdq_attention_f16_perceiver, mixdq_linear_f16_skinny; arithmetic: include/mixdq_math.h
// mixdq_perceiver_* / mixdq_skinny_*).  Both work on at most 16 rows per workgroup: one
// v_mfma_f32_16x16x32_f16 row block.
//
// mixdq_attention_f16_perceiver -- one softmax over the keys of TWO sources, 1 .. 16 queries per head.
//   ownership    a workgroup of four waves per (head, batch).  No K or V row is used twice, so nothing is staged in LDS.
//   keys         dealt to the waves in blocks of 32, round-robin: block j (keys 32 j .. 32 j + 31 of the concatenation,
//                wherever the seam between the sources falls) belongs to wave j % 4.
//   orientation  S^T = K Q^T: the MFMA's row index is a KEY, its column index a QUERY.  A lane (tk = lane % 16,
//                g = lane / 16) then holds, for query tk, the scores of keys 16 s + 4 g + r (s = 0, 1; r = 0 .. 3) of the
//                block: exactly the eight values the B operand of O^T = V^T P^T wants from it (the contraction index
//                of an MFMA may be permuted freely as long as both operands agree), so P never leaves its registers,
//                and the softmax state of query tk (running maximum, sum) lives in the lanes that hold its O column.
//   operands     K: a lane reads 16 bytes of key row tk -- straight into the A operand.  V: a lane reads the 8 bytes
//                d = 4 tk .. 4 tk + 3 of its eight keys (16 lanes cover one 128-byte head row) and eight v_perm_b32
//                turn them into the four A operands of the d tiles dt = 0 .. 3; output column tk of tile dt is
//                d = 4 tk + dt, so a lane ends with d = 16 g + 4 r + dt: four consecutive values per r.
//   combine      the four partial (max, sum, 16 x 64 accumulator) states meet once in LDS (16.5 KB) and are combined
//                in wave order by mixdq_perceiver_combine; a wave that received no block takes no part.
//
// mixdq_linear_f16_skinny -- D = [residual +] act(LN?(A) W^T + bias) for M <= 256 rows: weight streaming.
//   ownership    grid (N / 16, ceil(M / 16)); a workgroup of four waves owns a 16 x 16 output tile over all of K; wave w
//                takes the K steps of 32 with step % 4 == w, so the four waves read 256 consecutive bytes of a weight row.
//   operands     W rows are 16-byte loads straight into the A operand (the MFMA's row index is an output COLUMN, as in
//                clip_vision.hip: a lane ends with four consecutive columns of one row), kDepth = 8 of them in flight
//                per wave; the rows of A are the B operand: from global memory (L2) in the same pipeline, or -- with
//                the LayerNorm prologue -- from LDS, where the workgroup has normalised its 16 rows once, 16 lanes a row.
//   epilogue     the four K partials meet in LDS and are summed in wave order; bias, rounding, activation, residual.
#include "common.h"
#include "../../include/mixdq_math.h"

namespace mixdq {
namespace {

typedef unsigned short u16;

__device__ __forceinline__ float half_value(uint32_t bits) {
  __half_raw r;
  r.x = (unsigned short)(bits & 0xffffu);
  return __half2float(__half(r));
}

__device__ __forceinline__ v8h as_v8h(const uint4& w) { return __builtin_bit_cast(v8h, w); }

// ------------------------------------------------------------------------------------------------ perceiver attention

struct PerceiverArgs {
  const u16* q; const u16* k1; const u16* v1; const u16* k2; const u16* v2; u16* out;
  int64_t q_bs, q_rs, k1_bs, k1_rs, v1_bs, v1_rs, k2_bs, k2_rs, v2_bs, v2_rs, o_bs, o_rs;
  int tq, t1, t2;
  float scale_log2;                // softmax scale * log2(e): the exponentials are base 2 (v_exp_f32), as in attention.hip
};

__global__ __launch_bounds__(256) void attn_perceiver_kernel(PerceiverArgs p) {
  __shared__ __attribute__((aligned(16))) float o_part[4][16][64];
  __shared__ float m_part[4][16], l_part[4][16];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, tk = lane & 15, g = lane >> 4;
  const int h = blockIdx.x, b = blockIdx.y;
  const int T = p.t1 + p.t2, nblk = (T + 31) >> 5;
  const float c = p.scale_log2;

  // the row of key `key` (0 <= key < T) of K or V: source 1 up to the seam, source 2 behind it
  const u16* k1b = p.k1 + (int64_t)b * p.k1_bs + h * 64;
  const u16* v1b = p.v1 + (int64_t)b * p.v1_bs + h * 64;
  const u16* k2b = p.k2 + (int64_t)b * p.k2_bs + h * 64;
  const u16* v2b = p.v2 + (int64_t)b * p.v2_bs + h * 64;
  auto krow = [&](int key) { return key < p.t1 ? k1b + (int64_t)key * p.k1_rs : k2b + (int64_t)(key - p.t1) * p.k2_rs; };
  auto vrow = [&](int key) { return key < p.t1 ? v1b + (int64_t)key * p.v1_rs : v2b + (int64_t)(key - p.t1) * p.v2_rs; };

  // the query rows: the B operand of both K steps, held for the whole kernel; rows past tq are zeros
  v8h qf[2];
  {
    uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0;
    if (tk < p.tq) {
      const u16* qr = p.q + (int64_t)b * p.q_bs + (int64_t)tk * p.q_rs + h * 64 + g * 8;
      w0 = *reinterpret_cast<const uint4*>(qr);
      w1 = *reinterpret_cast<const uint4*>(qr + 32);
    }
    qf[0] = as_v8h(w0), qf[1] = as_v8h(w1);
  }

  float m_run = -INFINITY, l_run = 0.0f;         // of query tk, over this wave's blocks
  v4f acc[4];                                    // acc[dt][r] = O[tk][16 g + 4 r + dt]
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) acc[dt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};

  for (int blk = wave; blk < nblk; blk += 4) {
    const int kb = blk * 32;
    // ---- loads: K rows kb + 16 s + tk, V rows kb + 16 s + 4 g + r.  A key past T reads the last key's row (in
    // bounds); its score is masked and its V values are replaced by zeros.
    uint4 kw[2][2];
    uint2 vw[8];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int key = kb + 16 * s + tk;
      const u16* kr = krow(key < T ? key : T - 1) + g * 8;
      kw[s][0] = *reinterpret_cast<const uint4*>(kr);
      kw[s][1] = *reinterpret_cast<const uint4*>(kr + 32);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int key = kb + 16 * (e >> 2) + 4 * g + (e & 3);
      vw[e] = *reinterpret_cast<const uint2*>(vrow(key < T ? key : T - 1) + 4 * tk);
      if (key >= T) vw[e] = make_uint2(0, 0);
    }
    // ---- S^T = K Q^T
    v4f sc[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      sc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_v8h(kw[s][0]), qf[0], v4f{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
      sc[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_v8h(kw[s][1]), qf[1], sc[s], 0, 0, 0);
    }
    // ---- online softmax of query tk over this block: eight keys here, the rest in lanes tk + 16, + 32, + 48
    float bm = -INFINITY;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool ok = kb + 16 * (e >> 2) + 4 * g + (e & 3) < T;
      sc[e >> 2][e & 3] = ok ? sc[e >> 2][e & 3] : -INFINITY;
      bm = fmaxf(bm, sc[e >> 2][e & 3]);
    }
    bm = fmaxf(bm, __shfl_xor(bm, 16));
    bm = fmaxf(bm, __shfl_xor(bm, 32));
    const float m_new = fmaxf(m_run, bm);        // finite: a block that exists has at least one key
    const float mc = m_new * c;
    // the first block of a wave has nothing to rescale: said here, not left to exp2(-inf)
    const float alpha = m_run == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f((m_run - m_new) * c);
    v8h pf;
    float ls = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float s = sc[e >> 2][e & 3];
      const float pe = s == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(__builtin_fmaf(s, c, -mc));
      pf[e] = (_Float16)pe;
      ls = MIXDQ_ADD_RN(ls, (float)pf[e]);       // the sum is taken over the ROUNDED P, as in attention.hip
    }
    ls = MIXDQ_ADD_RN(ls, __shfl_xor(ls, 16));
    ls = MIXDQ_ADD_RN(ls, __shfl_xor(ls, 32));
    l_run = __builtin_fmaf(l_run, alpha, ls);
    m_run = m_new;
    // ---- O^T = alpha O^T + V^T P^T
    uint32_t vf[4][4];                           // [dt][j]: keys e = 2 j (low half) and 2 j + 1 (high half) at d = 4 tk + dt
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint2 a = vw[2 * j], bb = vw[2 * j + 1];
      vf[0][j] = __builtin_amdgcn_perm(bb.x, a.x, 0x05040100u);
      vf[1][j] = __builtin_amdgcn_perm(bb.x, a.x, 0x07060302u);
      vf[2][j] = __builtin_amdgcn_perm(bb.y, a.y, 0x05040100u);
      vf[3][j] = __builtin_amdgcn_perm(bb.y, a.y, 0x07060302u);
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[dt][r] = MIXDQ_MUL_RN(acc[dt][r], alpha);
      acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_v8h(make_uint4(vf[dt][0], vf[dt][1], vf[dt][2], vf[dt][3])), pf,
                                                       acc[dt], 0, 0, 0);
    }
  }

  // ---- the partial states meet.  A wave without a block writes nothing and is not read.
  if (wave < nblk) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      *reinterpret_cast<float4*>(&o_part[wave][tk][16 * g + 4 * r]) =
          make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
    if (g == 0) m_part[wave][tk] = m_run, l_part[wave][tk] = l_run;
  }
  __syncthreads();
  const int nw = nblk < 4 ? nblk : 4;
  const int row = tid >> 4, d0 = (tid & 15) * 4;
  if (row >= p.tq) return;
  float m_all = m_part[0][row];
  for (int w = 1; w < nw; ++w) m_all = fmaxf(m_all, m_part[w][row]);
  float wgt[4], lw[4], ow[4][4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    wgt[w] = 0.0f, lw[w] = 0.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) ow[w][e] = 0.0f;
    if (w < nw) {
      wgt[w] = __builtin_amdgcn_exp2f((m_part[w][row] - m_all) * c);
      lw[w] = l_part[w][row];
      const float4 o = *reinterpret_cast<const float4*>(&o_part[w][row][d0]);
      ow[w][0] = o.x, ow[w][1] = o.y, ow[w][2] = o.z, ow[w][3] = o.w;
    }
  }
  uint32_t y[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float o4[4] = {ow[0][e], ow[1][e], ow[2][e], ow[3][e]};
    y[e] = half_bits(mixdq_perceiver_combine(wgt, lw, o4, nw));
  }
  u16* orow = p.out + (int64_t)b * p.o_bs + (int64_t)row * p.o_rs + h * 64 + d0;
  *reinterpret_cast<uint2*>(orow) = make_uint2(y[0] | (y[1] << 16), y[2] | (y[3] << 16));
}

// ------------------------------------------------------------------------------------------------------- skinny GEMM

constexpr int kDepth = 8;                        // weight (and A) loads in flight per wave
constexpr int kLnMaxK = MIXDQ_SKINNY_LN_MAX_K;   // 2048: 16 rows x (2048 + 8) halves = 64.25 KB of LDS

struct SkinnyArgs {
  const u16* A; const u16* W; const u16* bias; const u16* res; u16* D;
  const u16* ln_w; const u16* ln_b;
  int64_t lda, ldd;
  float eps;
  int M, N, K;
};

template <bool LN, bool GELU>
__global__ __launch_bounds__(256) void linear_skinny_kernel(SkinnyArgs p) {
  extern __shared__ __attribute__((aligned(16))) u16 a_rows[];     // LN: [16][K + 8]
  __shared__ __attribute__((aligned(16))) float part[4][16][16];  // [wave][row][column]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, tk = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
  const int K = p.K, nsteps = K >> 5, pitch = K + 8;
  const int cnt = (nsteps - wave + 3) >> 2;      // this wave's K steps: wave, wave + 4, ...

  // a step past the wave's last one reads the row's last step again (in bounds) and is not used
  const u16* wrow = p.W + (int64_t)(n0 + tk) * K + g * 8;
  auto wload = [&](int i) {
    int s = wave + 4 * i;
    s = s < nsteps ? s : nsteps - 1;
    return *reinterpret_cast<const uint4*>(wrow + s * 32);
  };
  const int mrow = m0 + tk < p.M ? m0 + tk : p.M - 1;      // a row past M reads row M - 1 and is not stored
  const u16* arow = p.A + (int64_t)mrow * p.lda + g * 8;
  auto aload = [&](int i) {
    int s = wave + 4 * i;
    s = s < nsteps ? s : nsteps - 1;
    return *reinterpret_cast<const uint4*>(arow + s * 32);
  };

  uint4 wf[kDepth], af[kDepth];
#pragma unroll
  for (int u = 0; u < kDepth; ++u) {             // the weight stream starts before the prologue
    wf[u] = wload(u);
    if constexpr (!LN) af[u] = aload(u);
  }

  if constexpr (LN) {
    // ---- the LayerNorm prologue: 16 lanes per row; lane cl owns the 8-element chunks cl, cl + 16, ... of its row.
    // Pass 1 copies the row into LDS and sums it, pass 2 sums the squared deviations, pass 3 normalises in place: a
    // lane only ever reads LDS chunks it wrote itself, so the passes need no barrier between them.
    const int r = tid >> 4, cl = tid & 15, chunks = K >> 3;
    const int gr = m0 + r < p.M ? m0 + r : p.M - 1;
    const u16* src = p.A + (int64_t)gr * p.lda;
    u16* dst = a_rows + r * pitch;
    float s = 0.0f;
    for (int ch = cl; ch < chunks; ch += 16) {
      const Half8 x = *reinterpret_cast<const Half8*>(src + ch * 8);
      *reinterpret_cast<Half8*>(dst + ch * 8) = x;
#pragma unroll
      for (int e = 0; e < 8; ++e) s = MIXDQ_ADD_RN(s, half_at(x, e));
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) s = MIXDQ_ADD_RN(s, __shfl_xor(s, o));
    const float mean = mixdq_clip_ln_mean(s, K);
    float ss = 0.0f;
    for (int ch = cl; ch < chunks; ch += 16) {
      const Half8 x = *reinterpret_cast<const Half8*>(dst + ch * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) ss = mixdq_clip_ln_sq(half_at(x, e), mean, ss);
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) ss = MIXDQ_ADD_RN(ss, __shfl_xor(ss, o));
    const float rstd = mixdq_clip_ln_rstd(ss, K, p.eps);
    for (int ch = cl; ch < chunks; ch += 16) {
      const Half8 x = *reinterpret_cast<const Half8*>(dst + ch * 8);
      const Half8 gm = *reinterpret_cast<const Half8*>(p.ln_w + ch * 8);
      const Half8 bt = *reinterpret_cast<const Half8*>(p.ln_b + ch * 8);
      Half8 y;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t lo = half_bits(mixdq_clip_ln_apply(half_at(x, 2 * e), mean, rstd, half_at(gm, 2 * e), half_at(bt, 2 * e)));
        const uint32_t hi = half_bits(mixdq_clip_ln_apply(half_at(x, 2 * e + 1), mean, rstd, half_at(gm, 2 * e + 1), half_at(bt, 2 * e + 1)));
        y.w[e] = lo | (hi << 16);
      }
      *reinterpret_cast<Half8*>(dst + ch * 8) = y;
    }
    __syncthreads();
  }

  // ---- the product: acc[r] = sum over this wave's steps of W[n0 + 4 g + r, k] * A[m0 + tk, k]
  v4f acc = v4f{0.0f, 0.0f, 0.0f, 0.0f};
  const u16* xrow = a_rows + tk * pitch + g * 8;
  for (int base = 0; base < cnt; base += kDepth) {
#pragma unroll
    for (int u = 0; u < kDepth; ++u) {
      const int i = base + u;
      if (i < cnt) {                             // (wave-uniform)
        uint4 x;
        if constexpr (LN) x = *reinterpret_cast<const uint4*>(xrow + (wave + 4 * i) * 32);
        else x = af[u];
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(as_v8h(wf[u]), as_v8h(x), acc, 0, 0, 0);
        if (i + kDepth < cnt) {
          wf[u] = wload(i + kDepth);
          if constexpr (!LN) af[u] = aload(i + kDepth);
        }
      }
    }
  }

  // ---- the K partials meet (a wave without a step brings zeros); 64 lanes finish four columns of one row each
  *reinterpret_cast<float4*>(&part[wave][tk][4 * g]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  __syncthreads();
  if (tid >= 64) return;
  const int r = tid >> 2, c4 = (tid & 3) * 4, m = m0 + r, n = n0 + c4;
  if (m >= p.M) return;
  float4 pw[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) pw[w] = *reinterpret_cast<const float4*>(&part[w][r][c4]);
  float bs[4] = {0.0f, 0.0f, 0.0f, 0.0f}, rs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const bool has_bias = p.bias != nullptr, has_res = p.res != nullptr;
  if (has_bias) {
    const uint2 t = *reinterpret_cast<const uint2*>(p.bias + n);
    bs[0] = half_value(t.x), bs[1] = half_value(t.x >> 16), bs[2] = half_value(t.y), bs[3] = half_value(t.y >> 16);
  }
  if (has_res) {                                 // read here, written below by the same lane: D may be the residual
    const uint2 t = *reinterpret_cast<const uint2*>(p.res + (int64_t)m * p.ldd + n);
    rs[0] = half_value(t.x), rs[1] = half_value(t.x >> 16), rs[2] = half_value(t.y), rs[3] = half_value(t.y >> 16);
  }
  const float s4[4] = {mixdq_skinny_sum(pw[0].x, pw[1].x, pw[2].x, pw[3].x), mixdq_skinny_sum(pw[0].y, pw[1].y, pw[2].y, pw[3].y),
                       mixdq_skinny_sum(pw[0].z, pw[1].z, pw[2].z, pw[3].z), mixdq_skinny_sum(pw[0].w, pw[1].w, pw[2].w, pw[3].w)};
  uint32_t y[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float v = half_value(half_bits(has_bias ? mixdq_skinny_bias(s4[e], bs[e]) : s4[e]));
    if constexpr (GELU) v = half_value(half_bits(mixdq_geluf(v)));
    if (has_res) v = half_value(half_bits(mixdq_skinny_residual(v, rs[e])));
    y[e] = half_bits(v);
  }
  *reinterpret_cast<uint2*>(p.D + (int64_t)m * p.ldd + n) = make_uint2(y[0] | (y[1] << 16), y[2] | (y[3] << 16));
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

inline bool overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)b_bytes && y < x + (uintptr_t)a_bytes;
}

template <bool LN, bool GELU>
int launch_skinny(const SkinnyArgs& a, hipStream_t stream) {
  int lds = 0;
  if constexpr (LN) {
    lds = 16 * (a.K + 8) * 2;
    const int st = lds_opt_in<linear_skinny_kernel<LN, GELU>>(16 * (kLnMaxK + 8) * 2);
    if (st != MIXDQ_OK) return st;
  }
  const dim3 grid((unsigned)(a.N / 16), (unsigned)((a.M + 15) / 16));
  hipLaunchKernelGGL((linear_skinny_kernel<LN, GELU>), grid, dim3(256), lds, stream, a);
  return launch_status();
}

}  // namespace
}  // namespace mixdq

extern "C" int mixdq_attention_f16_perceiver(const void* q_f16, const void* k1_f16, const void* v1_f16,
                                             const void* k2_f16, const void* v2_f16, void* out_f16, int batch, int heads,
                                             int head_dim, int tq, int t1, int t2, int64_t q_batch_stride,
                                             int64_t q_row_stride, int64_t k1_batch_stride, int64_t k1_row_stride,
                                             int64_t v1_batch_stride, int64_t v1_row_stride, int64_t k2_batch_stride,
                                             int64_t k2_row_stride, int64_t v2_batch_stride, int64_t v2_row_stride,
                                             int64_t out_batch_stride, int64_t out_row_stride, float softmax_scale,
                                             mixdq_stream_t stream) {
  using namespace mixdq;
  if (batch < 0 || batch > 65535 || heads <= 0) return MIXDQ_ERR_INVALID_ARG;
  if (head_dim != 64 || tq < 1 || tq > MIXDQ_PERCEIVER_MAX_Q || t1 < 1 || t2 < 0 ||
      (int64_t)t1 + t2 > MIXDQ_PERCEIVER_MAX_KEYS)
    return MIXDQ_ERR_SHAPE;
  if (!q_f16 || !k1_f16 || !v1_f16 || !out_f16 || (t2 > 0 && (!k2_f16 || !v2_f16))) return MIXDQ_ERR_INVALID_ARG;
  const int64_t strides[] = {q_batch_stride, q_row_stride, k1_batch_stride, k1_row_stride, v1_batch_stride, v1_row_stride,
                             k2_batch_stride, k2_row_stride, v2_batch_stride, v2_row_stride, out_batch_stride,
                             out_row_stride};
  for (int64_t s : strides)
    if (s % 8) return MIXDQ_ERR_ALIGNMENT;
  if (((uintptr_t)q_f16 | (uintptr_t)k1_f16 | (uintptr_t)v1_f16 | (uintptr_t)k2_f16 | (uintptr_t)v2_f16 |
       (uintptr_t)out_f16) & 15)
    return MIXDQ_ERR_ALIGNMENT;
  if (batch == 0) return MIXDQ_OK;
  PerceiverArgs a;
  a.q = (const u16*)q_f16, a.k1 = (const u16*)k1_f16, a.v1 = (const u16*)v1_f16;
  a.k2 = (const u16*)(t2 > 0 ? k2_f16 : k1_f16), a.v2 = (const u16*)(t2 > 0 ? v2_f16 : v1_f16);   // (never read at t2 == 0)
  a.out = (u16*)out_f16;
  a.q_bs = q_batch_stride, a.q_rs = q_row_stride, a.k1_bs = k1_batch_stride, a.k1_rs = k1_row_stride;
  a.v1_bs = v1_batch_stride, a.v1_rs = v1_row_stride, a.k2_bs = k2_batch_stride, a.k2_rs = k2_row_stride;
  a.v2_bs = v2_batch_stride, a.v2_rs = v2_row_stride, a.o_bs = out_batch_stride, a.o_rs = out_row_stride;
  a.tq = tq, a.t1 = t1, a.t2 = t2;
  a.scale_log2 = softmax_scale * 1.44269504088896341f;
  hipLaunchKernelGGL(attn_perceiver_kernel, dim3((unsigned)heads, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
  return launch_status();
}

extern "C" int mixdq_linear_f16_skinny(const void* A_f16, int64_t lda, const void* W_f16, const void* bias_f16_or_null,
                                       const void* residual_f16_or_null, void* D_f16, int64_t ldd, int M, int N, int K,
                                       const void* ln_weight_f16_or_null, const void* ln_bias_f16_or_null, float eps,
                                       int flags, mixdq_stream_t stream) {
  using namespace mixdq;
  if (!A_f16 || !W_f16 || !D_f16 || (ln_weight_f16_or_null == nullptr) != (ln_bias_f16_or_null == nullptr))
    return MIXDQ_ERR_INVALID_ARG;
  if (flags & ~MIXDQ_FLAG_ACT_GELU) return MIXDQ_ERR_UNSUPPORTED;
  const bool ln = ln_weight_f16_or_null != nullptr;
  if (M < 1 || M > MIXDQ_SKINNY_MAX_M || N < 16 || N % 16 != 0 || K < 32 || K % 32 != 0 || K > MIXDQ_SKINNY_MAX_K ||
      (ln && K > MIXDQ_SKINNY_LN_MAX_K) || lda < K || ldd < N)
    return MIXDQ_ERR_SHAPE;
  if (lda % 8 != 0 || ldd % 4 != 0 || !aligned(A_f16, 16) || !aligned(W_f16, 16) || !aligned(D_f16, 8) ||
      !aligned(bias_f16_or_null, 8) || !aligned(residual_f16_or_null, 8) || !aligned(ln_weight_f16_or_null, 16) ||
      !aligned(ln_bias_f16_or_null, 16))
    return MIXDQ_ERR_ALIGNMENT;
  // D is written while other workgroups still read A: they may not share memory (the residual may be D itself)
  const int64_t d_bytes = (((int64_t)M - 1) * ldd + N) * 2;
  if (overlap(A_f16, (((int64_t)M - 1) * lda + K) * 2, D_f16, d_bytes)) return MIXDQ_ERR_INVALID_ARG;
  // ... and a residual that overlaps D without being D would be read by one lane after another wrote it
  if (residual_f16_or_null && residual_f16_or_null != D_f16 && overlap(residual_f16_or_null, d_bytes, D_f16, d_bytes))
    return MIXDQ_ERR_INVALID_ARG;
  SkinnyArgs a;
  a.A = (const u16*)A_f16, a.W = (const u16*)W_f16, a.bias = (const u16*)bias_f16_or_null;
  a.res = (const u16*)residual_f16_or_null, a.D = (u16*)D_f16;
  a.ln_w = (const u16*)ln_weight_f16_or_null, a.ln_b = (const u16*)ln_bias_f16_or_null;
  a.lda = lda, a.ldd = ldd, a.eps = eps, a.M = M, a.N = N, a.K = K;
  const bool gelu = (flags & MIXDQ_FLAG_ACT_GELU) != 0;
  hipStream_t s = (hipStream_t)stream;
  if (ln) return gelu ? launch_skinny<true, true>(a, s) : launch_skinny<true, false>(a, s);
  return gelu ? launch_skinny<false, true>(a, s) : launch_skinny<false, false>(a, s);
}
