// LoHa and DoRA on quantized layers: W' = g (.) (W + sum_lin s_j B_j A_j + sum_had s_j (B1_j A1_j) (.) (B2_j A2_j)),
// g[n] = m[n] / ||row n||_2 (1 without a magnitude), re-quantized with the layer's own quantizer and written in place
// into the buffers the GEMM / conv kernels read -- every targeted layer of a network in ONE launch
// (include/mixdq_hip.h mixdq_lycoris_requant; arithmetic: include/mixdq_math.h mixdq_lycoris_*).
//
// A kernel of its own, built to csrc/lora.hip's plan; what it shares with it is restated, not included, so that unit's
// kernels stay what they are.
//
//   ownership    as lora.hip: a workgroup of four waves owns 16 output rows over the WHOLE Kf, so the row maximum, the
//                row sums, the scale AND the row's sum of squares never leave it.  A trip covers 4 waves x 64 columns;
//                column = 16 g + 4 cb + e, so a lane holds 16 consecutive columns of one row (row = lane % 16).
//   linear       ranks [0, R_lin): lora.hip's loop, MFMA by MFMA, into accumulators that start as the master tile --
//                a table with no Hadamard term and no magnitude writes lora_requant's bytes.
//   Hadamard     term t owns ranks [had_end[t - 1], had_end[t]) (the first starts at R_lin), a multiple of 32.  Per trip
//                and term two zero-initialised accumulator sets P1 = Bs1 A1, P2 = B2 A2 run over the term's 32-rank
//                pieces side by side; then acc = fma(P1, P2, acc) per element, terms in table order.  48 accumulator
//                registers per lane in all.
//   staging      two Bs images of the 16 rows (Bs1 = f16(svec * Bcat), B2 as it is; 2 x 8.25 KB, once per workgroup)
//                and two transposed A pieces (2 x 20 KB, per 32 ranks, behind the same two barriers): 56.5 KB of LDS.
//   the norm     a magnitude forces the first pass even under KEEP: it takes max |w'| and sum w'^2 per lane, reduced
//                over the four lane groups by __shfl_xor and over the waves through LDS.  g = m / sqrt(sumsq), both
//                correctly rounded; the second pass recomputes the product and quantizes mul_rn(g, w'); ABSMAX takes
//                its delta from mul_rn(|g|, max |w'|) -- rounding is monotonic, so that IS the scaled row's maximum.
//   stores       plain C++ vector stores; LDS integer adds for the per-tap sums.  No scratch.
#include "common.h"
#include "../../include/mixdq_math.h"

namespace mixdq {
namespace {

constexpr int kRows = MIXDQ_LORA_ROWS;   // rows per workgroup
constexpr int kTrip = 256;               // columns per trip (4 waves x 64)
constexpr int kRC = 32;                  // ranks per staged piece = one MFMA's reduction
constexpr int kAPitch = 40;              // halves per column of a transposed A piece (80 bytes: 16-byte reads)
constexpr int kBPitch = 264;             // halves per row of a Bs image (528 bytes)
constexpr int kMaxTaps = 16;

struct alignas(8) Half4 { uint32_t w[2]; };

__device__ __forceinline__ float half_lo(uint32_t w) {
  __half_raw r;
  r.x = (unsigned short)(w & 0xffffu);
  return __half2float(__half(r));
}
__device__ __forceinline__ float half_hi(uint32_t w) {
  __half_raw r;
  r.x = (unsigned short)(w >> 16);
  return __half2float(__half(r));
}

// One [32 ranks][256 columns] piece of a factor A [R, Kf], rows r0 .. r0 + 31 and columns k0 .. k0 + 255 (zeros past
// Kf), read with coalesced 8-byte loads and written transposed: at[column][rank].
__device__ __forceinline__ void stage_piece(_Float16* __restrict__ at, const __half* __restrict__ A, int r0, int k0, int Kf,
                                            int tid) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {                               // [32 ranks][64 groups of 4 columns]
    const int idx = tid + 256 * i, rr = idx >> 6, c4 = idx & 63;
    Half4 a = {{0u, 0u}};
    if (k0 + c4 * 4 < Kf) a = *reinterpret_cast<const Half4*>(A + (int64_t)(r0 + rr) * Kf + k0 + c4 * 4);
    unsigned short* dst = reinterpret_cast<unsigned short*>(at) + (c4 * 4) * kAPitch + rr;
    dst[0] = (unsigned short)(a.w[0] & 0xffffu);
    dst[kAPitch] = (unsigned short)(a.w[0] >> 16);
    dst[2 * kAPitch] = (unsigned short)(a.w[1] & 0xffffu);
    dst[3 * kAPitch] = (unsigned short)(a.w[1] >> 16);
  }
}

__global__ __launch_bounds__(256) void lycoris_requant_kernel(const mixdq_lycoris_layer* __restrict__ layers,
                                                              const int32_t* __restrict__ prefix, int n_layers) {
  __shared__ __attribute__((aligned(16))) _Float16 at[2][kTrip * kAPitch];   // 2 x 20 KB
  __shared__ __attribute__((aligned(16))) _Float16 bs[2][kRows * kBPitch];   // 2 x 8.25 KB
  __shared__ float row_max[4][kRows];
  __shared__ float row_ss[4][kRows];
  __shared__ float delta_s[kRows];
  __shared__ int row_sum[kRows][kMaxTaps];

  // ---- which layer: the last i with prefix[i] <= block
  const int block = blockIdx.x;
  int lo = 0, hi = n_layers;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= block) lo = mid;
    else hi = mid;
  }
  // (the descriptor stays in memory: its fields are read one by one, had_end[] by a run-time index)
  const mixdq_lycoris_layer* __restrict__ L = layers + lo;
  const int N = L->N, Kf = L->Kf, R = L->R, R_lin = L->R_lin, n_had = L->n_had;
  const int mode = L->mode, rule = L->rule, bits = L->bits, tap_len = L->tap_len;
  const int row0 = (block - prefix[lo]) * kRows;
  if (row0 >= N) return;                                      // (a table that disagrees with its prefix: nothing)

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nl = lane & 15, g = lane >> 4;
  const int n = row0 + nl;
  const bool row_ok = n < N;
  const int32_t* row_map = L->row_map;
  const int srow = row_ok ? (row_map ? row_map[n] : n) : 0;
  const int taps = Kf / tap_len;
  const bool integer = mode != MIXDQ_LORA_F16;
  const __half* A1 = (const __half*)L->Acat;
  const __half* A2 = (const __half*)L->A2cat;
  const float* magnitude = L->magnitude;

  // ---- the two Bs images of the block's rows, once: 16 rows x R ranks, four ranks per item
  {
    const __half* B1 = (const __half*)L->Bcat;
    const __half* B2 = (const __half*)L->B2cat;
    const float* svec = L->svec;
    for (int item = tid; item < kRows * (R >> 2); item += 256) {
      const int r4 = item % (R >> 2), rr = item / (R >> 2);
      Half4 b = {{0u, 0u}}, b2 = {{0u, 0u}};
      if (row0 + rr < N) {
        b = *reinterpret_cast<const Half4*>(B1 + (int64_t)(row0 + rr) * R + r4 * 4);
        if (n_had > 0) b2 = *reinterpret_cast<const Half4*>(B2 + (int64_t)(row0 + rr) * R + r4 * 4);
      }
      const float4 s = *reinterpret_cast<const float4*>(svec + r4 * 4);
      const uint32_t w0 = half_bits(mixdq_lora_scaled(s.x, half_lo(b.w[0]))) | (half_bits(mixdq_lora_scaled(s.y, half_hi(b.w[0]))) << 16);
      const uint32_t w1 = half_bits(mixdq_lora_scaled(s.z, half_lo(b.w[1]))) | (half_bits(mixdq_lora_scaled(s.w, half_hi(b.w[1]))) << 16);
      *reinterpret_cast<uint2*>(bs[0] + rr * kBPitch + r4 * 4) = make_uint2(w0, w1);
      *reinterpret_cast<uint2*>(bs[1] + rr * kBPitch + r4 * 4) = make_uint2(b2.w[0], b2.w[1]);
    }
  }
  for (int i = tid; i < kRows * kMaxTaps; i += 256) (&row_sum[0][0])[i] = 0;
  __syncthreads();                                            // (a layer may have no rank piece in front of its first read)

  const __half* wrow = (const __half*)L->W + (int64_t)n * L->ldw + L->w_col0;
  const int qmax = (1 << (bits - 1)) - 1, qmin = -qmax - 1;
  float delta = 1.0f, gain = 1.0f;
  if (integer && row_ok) delta = L->weight_scales[srow];

  const bool absmax = integer && rule == MIXDQ_LORA_ABSMAX;
  const int first_pass = (absmax || magnitude) ? 0 : 1;
  for (int pass = first_pass; pass < 2; ++pass) {
    float m = 0.0f, ss = 0.0f;
    int tap = 0, tap_end = tap_len, s_tap = 0;
    for (int k0 = 0; k0 < Kf; k0 += kTrip) {
      const int col = k0 + wave * 64 + g * 16;                // this lane's 16 consecutive columns
      // ---- the accumulators start as the master tile
      v4f acc[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        Half4 w = {{0u, 0u}};
        if (row_ok && col + cb * 4 < Kf) w = *reinterpret_cast<const Half4*>(wrow + col + cb * 4);
        acc[cb] = v4f{half_lo(w.w[0]), half_hi(w.w[0]), half_lo(w.w[1]), half_hi(w.w[1])};
      }
      // ---- + Bs Acat over the linear ranks, 32 at a time
      for (int r0 = 0; r0 < R_lin; r0 += kRC) {
        __syncthreads();                                      // the previous piece's readers are done
        stage_piece(at[0], A1, r0, k0, Kf, tid);
        __syncthreads();
        const v8h b = *reinterpret_cast<const v8h*>(bs[0] + nl * kBPitch + r0 + g * 8);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          // MFMA row i = lane % 16 stands for column 16 (i / 4) + 4 cb + i % 4 of the wave's 64
          const int ca = wave * 64 + (nl >> 2) * 16 + cb * 4 + (nl & 3);
          const v8h a = *reinterpret_cast<const v8h*>(at[0] + ca * kAPitch + g * 8);
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[cb], 0, 0, 0);
        }
      }
      // ---- + (Bs1 A1) (.) (B2 A2), term by term
      int r_begin = R_lin;
      for (int t = 0; t < n_had; ++t) {
        const int r_end = L->had_end[t];
        v4f p1[4], p2[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) p1[cb] = v4f{0.0f, 0.0f, 0.0f, 0.0f}, p2[cb] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        for (int r0 = r_begin; r0 < r_end; r0 += kRC) {
          __syncthreads();
          stage_piece(at[0], A1, r0, k0, Kf, tid);
          stage_piece(at[1], A2, r0, k0, Kf, tid);
          __syncthreads();
          const v8h b1 = *reinterpret_cast<const v8h*>(bs[0] + nl * kBPitch + r0 + g * 8);
          const v8h b2 = *reinterpret_cast<const v8h*>(bs[1] + nl * kBPitch + r0 + g * 8);
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) {
            const int ca = wave * 64 + (nl >> 2) * 16 + cb * 4 + (nl & 3);
            const v8h a1 = *reinterpret_cast<const v8h*>(at[0] + ca * kAPitch + g * 8);
            const v8h a2 = *reinterpret_cast<const v8h*>(at[1] + ca * kAPitch + g * 8);
            p1[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b1, p1[cb], 0, 0, 0);
            p2[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2, b2, p2[cb], 0, 0, 0);
          }
        }
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[cb][e] = mixdq_lycoris_hadamard(p1[cb][e], p2[cb][e], acc[cb][e]);
        r_begin = r_end;
      }
      // ---- the tile: lane holds the unscaled w'[n, col + 4 cb + e] in acc[cb][e] (zeros past Kf and past N)
      if (pass == 0) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            m = fmaxf(m, fabsf(acc[cb][e]));
            ss = mixdq_lycoris_sumsq(acc[cb][e], ss);
          }
        continue;
      }
      if (!row_ok) continue;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[cb][e] = mixdq_lycoris_scaled(gain, acc[cb][e]);
      if (mode == MIXDQ_LORA_F16) {
        __half* orow = (__half*)L->out + (int64_t)srow * Kf;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
          if (col + cb * 4 < Kf)
            *reinterpret_cast<uint2*>(orow + col + cb * 4) =
                make_uint2(half_bits(acc[cb][0]) | (half_bits(acc[cb][1]) << 16),
                           half_bits(acc[cb][2]) | (half_bits(acc[cb][3]) << 16));
        continue;
      }
      int q[16];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        int s4 = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int v = (int)mixdq_lora_q(acc[cb][e], delta, bits);
          q[cb * 4 + e] = min(max(v, qmin), qmax);
          s4 += q[cb * 4 + e];
        }
        if (col + cb * 4 < Kf) {                              // (columns past Kf hold q = 0 of zeros: not counted anyway)
          while (col + cb * 4 >= tap_end) {
            atomicAdd(&row_sum[nl][tap], s_tap);
            s_tap = 0, ++tap, tap_end += tap_len;
          }
          s_tap += s4;
        }
      }
      if (mode == MIXDQ_LORA_INT8) {
        int8_t* orow = (int8_t*)L->out + (int64_t)srow * Kf;
        uint32_t d[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
          d[cb] = (uint32_t)(q[cb * 4] & 0xff) | ((uint32_t)(q[cb * 4 + 1] & 0xff) << 8) |
                  ((uint32_t)(q[cb * 4 + 2] & 0xff) << 16) | ((uint32_t)(q[cb * 4 + 3] & 0xff) << 24);
        if ((Kf & 15) == 0 && col < Kf) {
          *reinterpret_cast<uint4*>(orow + col) = make_uint4(d[0], d[1], d[2], d[3]);
        } else {
#pragma unroll
          for (int cb = 0; cb < 4; ++cb)
            if (col + cb * 4 < Kf) *reinterpret_cast<uint32_t*>(orow + col + cb * 4) = d[cb];
        }
      } else if (col < Kf) {                                  // W4: Kf % 32 == 0, the lane's 16 columns are all there
        // within 8 consecutive k, byte j holds k[j] in the high and k[4 + j] in the low nibble
        uint32_t d[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          uint32_t w = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            w |= ((((uint32_t)q[h * 8 + j] & 0xfu) << 4) | ((uint32_t)q[h * 8 + 4 + j] & 0xfu)) << (8 * j);
          d[h] = w;
        }
        *reinterpret_cast<uint2*>((int8_t*)L->out + (int64_t)srow * (Kf >> 1) + (col >> 1)) = make_uint2(d[0], d[1]);
      }
    }
    if (pass == 0) {
      // ---- the row's maximum and sum of squares: over the four lane groups, then over the four waves in order; every
      // lane derives its own row's gain and delta
      m = fmaxf(m, __shfl_xor(m, 16));
      m = fmaxf(m, __shfl_xor(m, 32));
      ss = MIXDQ_ADD_RN(ss, __shfl_xor(ss, 16));
      ss = MIXDQ_ADD_RN(ss, __shfl_xor(ss, 32));
      if (g == 0) row_max[wave][nl] = m, row_ss[wave][nl] = ss;
      __syncthreads();
      const float mx = fmaxf(fmaxf(row_max[0][nl], row_max[1][nl]), fmaxf(row_max[2][nl], row_max[3][nl]));
      const float sumsq = MIXDQ_ADD_RN(MIXDQ_ADD_RN(MIXDQ_ADD_RN(row_ss[0][nl], row_ss[1][nl]), row_ss[2][nl]), row_ss[3][nl]);
      if (magnitude && row_ok) gain = mixdq_lycoris_gain(magnitude[n], sumsq);
      if (absmax) delta = mixdq_lora_delta(mixdq_lycoris_scaled(fabsf(gain), mx), bits, delta);
    } else if (integer && row_ok) {
      atomicAdd(&row_sum[nl][tap], s_tap);
    }
  }
  if (!integer) return;
  if (wave == 0 && g == 0) delta_s[nl] = delta;
  __syncthreads();
  // ---- the per-channel vectors from_float computes from a weight, at the stored row
  if (tid < kRows && row0 + tid < N) {
    const int sr = row_map ? row_map[row0 + tid] : row0 + tid;
    float* wsum = L->wsum;
    float* bias0 = L->bias0;
    int total = 0;
    for (int t = 0; t < taps; ++t) {
      total += row_sum[tid][t];
      if (wsum) wsum[(int64_t)sr * taps + t] = (float)row_sum[tid][t];
    }
    const float d = delta_s[tid];
    if (bias0) bias0[sr] = MIXDQ_MUL_RN((float)total, L->act_zero_point[0]);
    if (rule == MIXDQ_LORA_ABSMAX) L->weight_scales[sr] = d;
    L->scale[sr] = MIXDQ_MUL_RN(d, L->act_scale[0]);
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int layer_status(const mixdq_lycoris_layer& L) {
  if (!L.W || !L.Bcat || !L.Acat || !L.svec || !L.out || L.N < 1 || L.Kf < 1) return MIXDQ_ERR_INVALID_ARG;
  if (L.mode == MIXDQ_LORA_W2) return MIXDQ_ERR_SHAPE;
  if (L.mode < 0 || L.mode > MIXDQ_LORA_W2 || (L.rule != MIXDQ_LORA_KEEP && L.rule != MIXDQ_LORA_ABSMAX))
    return MIXDQ_ERR_INVALID_ARG;
  if (L.mode == MIXDQ_LORA_INT8 && L.bits != 8 && L.bits != 4 && L.bits != 2) return MIXDQ_ERR_INVALID_ARG;
  if (L.mode == MIXDQ_LORA_W4 && L.bits != 4 && L.bits != 2) return MIXDQ_ERR_INVALID_ARG;
  if (L.mode != MIXDQ_LORA_F16 && (!L.weight_scales || !L.scale || !L.act_scale || !L.act_zero_point))
    return MIXDQ_ERR_INVALID_ARG;
  if (L.n_had < 0 || L.n_had > MIXDQ_LYCORIS_MAX_HADAMARD) return MIXDQ_ERR_INVALID_ARG;
  if (L.n_had > 0 && (!L.B2cat || !L.A2cat)) return MIXDQ_ERR_INVALID_ARG;
  if (L.R % 32 != 0 || L.R < 32 || L.R > 256 || L.Kf % 4 != 0) return MIXDQ_ERR_SHAPE;
  // the rank ranges: [0, R_lin), then one per Hadamard term, each a positive multiple of 32, all inside R
  if (L.R_lin % 32 != 0 || L.R_lin < 0 || L.R_lin > L.R) return MIXDQ_ERR_SHAPE;
  int begin = L.R_lin;
  for (int t = 0; t < L.n_had; ++t) {
    if (L.had_end[t] <= begin || (L.had_end[t] - begin) % 32 != 0 || L.had_end[t] > L.R) return MIXDQ_ERR_SHAPE;
    begin = L.had_end[t];
  }
  if (L.mode == MIXDQ_LORA_W4 && L.Kf % 32 != 0) return MIXDQ_ERR_SHAPE;
  if (L.tap_len < 4 || L.tap_len % 4 != 0 || L.Kf % L.tap_len != 0 || L.Kf / L.tap_len > kMaxTaps) return MIXDQ_ERR_SHAPE;
  if (L.ldw % 4 != 0 || L.w_col0 % 4 != 0 || L.w_col0 < 0 || L.ldw < 0) return MIXDQ_ERR_SHAPE;
  if (!aligned(L.W, 8) || !aligned(L.Bcat, 8) || !aligned(L.Acat, 8) || !aligned(L.svec, 16) || !aligned(L.out, 16))
    return MIXDQ_ERR_SHAPE;
  if (!aligned(L.B2cat, 8) || !aligned(L.A2cat, 8) || !aligned(L.magnitude, 4)) return MIXDQ_ERR_SHAPE;
  if (!aligned(L.row_map, 4) || !aligned(L.weight_scales, 4) || !aligned(L.wsum, 4) || !aligned(L.bias0, 4) ||
      !aligned(L.scale, 4) || !aligned(L.act_scale, 4) || !aligned(L.act_zero_point, 4))
    return MIXDQ_ERR_SHAPE;
  return MIXDQ_OK;
}

}  // namespace
}  // namespace mixdq

extern "C" int mixdq_lycoris_table(const mixdq_lycoris_layer* layers, int n_layers, int32_t* order, int32_t* prefix) {
  if (!layers || !order || !prefix || n_layers < 1) return -MIXDQ_ERR_INVALID_ARG;
  for (int i = 0; i < n_layers; ++i) {                          // a stable insertion sort, largest Kf first
    if (layers[i].N < 1 || layers[i].Kf < 1) return -MIXDQ_ERR_INVALID_ARG;
    int j = i;
    for (; j > 0 && layers[order[j - 1]].Kf < layers[i].Kf; --j) order[j] = order[j - 1];
    order[j] = i;
  }
  int64_t blocks = 0;
  for (int i = 0; i < n_layers; ++i) {
    prefix[i] = (int32_t)blocks;
    blocks += (layers[order[i]].N + MIXDQ_LORA_ROWS - 1) / MIXDQ_LORA_ROWS;
    if (blocks > 0x7fffffff) return -MIXDQ_ERR_INVALID_ARG;
  }
  prefix[n_layers] = (int32_t)blocks;
  return (int)blocks;
}

extern "C" int mixdq_lycoris_status(const mixdq_lycoris_layer* layers_host, int n_layers) {
  if (!layers_host || n_layers < 1) return MIXDQ_ERR_INVALID_ARG;
  for (int i = 0; i < n_layers; ++i) {
    const int st = mixdq::layer_status(layers_host[i]);
    if (st != MIXDQ_OK) return st;
  }
  return MIXDQ_OK;
}

extern "C" int mixdq_lycoris_requant(const mixdq_lycoris_layer* layers_host, const mixdq_lycoris_layer* layers_device,
                                     const int32_t* prefix_device, int n_layers, mixdq_stream_t stream) {
  using namespace mixdq;
  if (!layers_device || !prefix_device) return MIXDQ_ERR_INVALID_ARG;
  const int st = mixdq_lycoris_status(layers_host, n_layers);
  if (st != MIXDQ_OK) return st;
  int64_t blocks = 0;
  for (int i = 0; i < n_layers; ++i) blocks += (layers_host[i].N + kRows - 1) / kRows;
  if (blocks > 0x7fffffff || !aligned(layers_device, 8) || !aligned(prefix_device, 4)) return MIXDQ_ERR_INVALID_ARG;
  hipLaunchKernelGGL(lycoris_requant_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, layers_device,
                     prefix_device, n_layers);
  return launch_status();
}
