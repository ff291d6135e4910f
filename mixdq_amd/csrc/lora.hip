// LoRA on quantized layers: W' = W + sum_j s_j B_j A_j, re-quantized with the layer's own quantizer and written in place
// into the buffers the GEMM / conv kernels read -- every targeted layer of a network in ONE launch (include/mixdq_hip.h
// mixdq_lora_requant; arithmetic: include/mixdq_math.h mixdq_lora_*).
//
// A kernel of its own, not a member of the GEMM family: its reduction dimension is the rank (<= 256) and its output is
// as large as its largest input, so it is a streaming kernel with a small product inside.
//
//   ownership    a workgroup of four waves owns MIXDQ_LORA_ROWS = 16 output rows over the WHOLE Kf: the row maximum, the
//                row sums and the scale never leave it.  The grid is the sum over the layers of their row blocks, longest
//                rows first; a workgroup finds its layer by a binary search of the prefix table.
//   orientation  D[i, j] = sum_r AcatT[i, r] * Bs[j, r] on v_mfma_f32_16x16x32_f16: the MFMA's row index i is a weight
//                COLUMN, its column index j a weight ROW, so the four accumulator registers of a lane run along k.  The map
//                from (lane group g, block cb, register e) to the column is ours to choose: column = 16 g + 4 cb + e makes
//                the 16 values a lane holds after four blocks 16 CONSECUTIVE columns of one row (row = lane % 16) -- one
//                16-byte INT8 store (4-byte ones where Kf % 16 != 0), one 8-byte W4 store, four 8-byte FP16 stores, the master read alike, and no
//                cross-lane step or LDS round trip for the packing.  A trip of the workgroup covers 4 waves x 64 columns.
//   staging      Bs = f16(svec * Bcat) of the 16 rows is converted once into 8 KB of LDS and serves both passes.  Acat
//                streams: per trip and per 32 ranks a [32, 256] piece is read with coalesced 8-byte loads and written
//                TRANSPOSED ([column][rank], 80-byte pitch), so that both MFMA operands are one 16-byte LDS read.  Acat is
//                shared by every workgroup of its layer and stays in L2 / Infinity Cache.
//   two passes   under ABSMAX the first pass only takes max |W'|; the second RECOMPUTES the product (R / 32 MFMAs per
//                16 x 16 tile against one more read of the master) instead of keeping 16 x Kf FP32 values.
//   stores       plain C++ vector stores; LDS integer adds for the per-tap sums.  No scratch.
#include "common.h"
#include "../../include/mixdq_math.h"

namespace mixdq {
namespace {

constexpr int kRows = MIXDQ_LORA_ROWS;   // rows per workgroup
constexpr int kTrip = 256;               // columns per trip (4 waves x 64)
constexpr int kRC = 32;                  // ranks per staged piece = one MFMA's reduction
constexpr int kAPitch = 40;              // halves per column of the transposed Acat piece (80 bytes: 16-byte reads)
constexpr int kBPitch = 264;             // halves per row of Bs (528 bytes)
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

__global__ __launch_bounds__(256) void lora_requant_kernel(const mixdq_lora_layer* __restrict__ layers,
                                                           const int32_t* __restrict__ prefix, int n_layers) {
  __shared__ __attribute__((aligned(16))) _Float16 at[kTrip * kAPitch];   // 20 KB
  __shared__ __attribute__((aligned(16))) _Float16 bs[kRows * kBPitch];   // 8.25 KB
  __shared__ float row_max[4][kRows];
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
  const mixdq_lora_layer L = layers[lo];
  const int row0 = (block - prefix[lo]) * kRows;
  if (row0 >= L.N) return;                                    // (a table that disagrees with its prefix: nothing)

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nl = lane & 15, g = lane >> 4;
  const int N = L.N, Kf = L.Kf, R = L.R;
  const int n = row0 + nl;
  const bool row_ok = n < N;
  const int srow = row_ok ? (L.row_map ? L.row_map[n] : n) : 0;
  const int taps = Kf / L.tap_len;
  const bool integer = L.mode != MIXDQ_LORA_F16;

  // ---- Bs of the block's rows, once: 16 rows x R ranks, four ranks per item
  for (int item = tid; item < kRows * (R >> 2); item += 256) {
    const int r4 = item % (R >> 2), rr = item / (R >> 2);
    Half4 b = {{0u, 0u}};
    if (row0 + rr < N) b = *reinterpret_cast<const Half4*>((const __half*)L.Bcat + (int64_t)(row0 + rr) * R + r4 * 4);
    const float4 s = *reinterpret_cast<const float4*>(L.svec + r4 * 4);
    const uint32_t w0 = half_bits(mixdq_lora_scaled(s.x, half_lo(b.w[0]))) | (half_bits(mixdq_lora_scaled(s.y, half_hi(b.w[0]))) << 16);
    const uint32_t w1 = half_bits(mixdq_lora_scaled(s.z, half_lo(b.w[1]))) | (half_bits(mixdq_lora_scaled(s.w, half_hi(b.w[1]))) << 16);
    *reinterpret_cast<uint2*>(bs + rr * kBPitch + r4 * 4) = make_uint2(w0, w1);
  }
  for (int i = tid; i < kRows * kMaxTaps; i += 256) (&row_sum[0][0])[i] = 0;
  // (the first barrier of the first trip orders these writes before their readers)

  const __half* wrow = (const __half*)L.W + (int64_t)n * L.ldw + L.w_col0;
  const int qmax = (1 << (L.bits - 1)) - 1, qmin = -qmax - 1;
  float delta = 1.0f;
  if (integer && row_ok) delta = L.weight_scales[srow];

  const int first_pass = (integer && L.rule == MIXDQ_LORA_ABSMAX) ? 0 : 1;
  for (int pass = first_pass; pass < 2; ++pass) {
    float m = 0.0f;
    int tap = 0, tap_end = L.tap_len, s_tap = 0;
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
      // ---- + Bs Acat over the rank, 32 ranks at a time
      for (int r0 = 0; r0 < R; r0 += kRC) {
        __syncthreads();                                      // the previous piece's readers are done
#pragma unroll
        for (int i = 0; i < 8; ++i) {                         // [32 ranks][64 groups of 4 columns], 8-byte loads
          const int idx = tid + 256 * i, rr = idx >> 6, c4 = idx & 63;
          Half4 a = {{0u, 0u}};
          if (k0 + c4 * 4 < Kf)
            a = *reinterpret_cast<const Half4*>((const __half*)L.Acat + (int64_t)(r0 + rr) * Kf + k0 + c4 * 4);
          unsigned short* dst = reinterpret_cast<unsigned short*>(at) + (c4 * 4) * kAPitch + rr;
          dst[0] = (unsigned short)(a.w[0] & 0xffffu);
          dst[kAPitch] = (unsigned short)(a.w[0] >> 16);
          dst[2 * kAPitch] = (unsigned short)(a.w[1] & 0xffffu);
          dst[3 * kAPitch] = (unsigned short)(a.w[1] >> 16);
        }
        __syncthreads();
        const v8h b = *reinterpret_cast<const v8h*>(bs + nl * kBPitch + r0 + g * 8);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          // MFMA row i = lane % 16 stands for column 16 (i / 4) + 4 cb + i % 4 of the wave's 64
          const int ca = wave * 64 + (nl >> 2) * 16 + cb * 4 + (nl & 3);
          const v8h a = *reinterpret_cast<const v8h*>(at + ca * kAPitch + g * 8);
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[cb], 0, 0, 0);
        }
      }
      // ---- the tile: lane holds W'[n, col + 4 cb + e] in acc[cb][e]
      if (pass == 0) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int e = 0; e < 4; ++e) m = fmaxf(m, fabsf(acc[cb][e]));
        continue;
      }
      if (!row_ok) continue;
      if (L.mode == MIXDQ_LORA_F16) {
        __half* orow = (__half*)L.out + (int64_t)srow * Kf;
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
          const int v = (int)mixdq_lora_q(acc[cb][e], delta, L.bits);
          q[cb * 4 + e] = min(max(v, qmin), qmax);
          s4 += q[cb * 4 + e];
        }
        if (col + cb * 4 < Kf) {                              // (columns past Kf hold q = 0 of zeros: not counted anyway)
          while (col + cb * 4 >= tap_end) {
            atomicAdd(&row_sum[nl][tap], s_tap);
            s_tap = 0, ++tap, tap_end += L.tap_len;
          }
          s_tap += s4;
        }
      }
      if (L.mode == MIXDQ_LORA_INT8) {
        int8_t* orow = (int8_t*)L.out + (int64_t)srow * Kf;
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
        *reinterpret_cast<uint2*>((int8_t*)L.out + (int64_t)srow * (Kf >> 1) + (col >> 1)) = make_uint2(d[0], d[1]);
      }
    }
    if (pass == 0) {
      // ---- the row maximum: over the four lane groups, then over the four waves; every lane derives its own row's delta
      m = fmaxf(m, __shfl_xor(m, 16));
      m = fmaxf(m, __shfl_xor(m, 32));
      if (g == 0) row_max[wave][nl] = m;
      __syncthreads();
      const float mx = fmaxf(fmaxf(row_max[0][nl], row_max[1][nl]), fmaxf(row_max[2][nl], row_max[3][nl]));
      delta = mixdq_lora_delta(mx, L.bits, delta);
    } else if (integer && row_ok) {
      atomicAdd(&row_sum[nl][tap], s_tap);
    }
  }
  if (!integer) return;
  if (wave == 0 && g == 0) delta_s[nl] = delta;
  __syncthreads();
  // ---- the per-channel vectors from_float computes from a weight, at the stored row
  if (tid < kRows && row0 + tid < N) {
    const int sr = L.row_map ? L.row_map[row0 + tid] : row0 + tid;
    int total = 0;
    for (int t = 0; t < taps; ++t) {
      total += row_sum[tid][t];
      if (L.wsum) L.wsum[(int64_t)sr * taps + t] = (float)row_sum[tid][t];
    }
    const float d = delta_s[tid];
    if (L.bias0) L.bias0[sr] = MIXDQ_MUL_RN((float)total, L.act_zero_point[0]);
    if (L.rule == MIXDQ_LORA_ABSMAX) L.weight_scales[sr] = d;
    L.scale[sr] = MIXDQ_MUL_RN(d, L.act_scale[0]);
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int layer_status(const mixdq_lora_layer& L) {
  if (!L.W || !L.Bcat || !L.Acat || !L.svec || !L.out || L.N < 1 || L.Kf < 1) return MIXDQ_ERR_INVALID_ARG;
  if (L.mode == MIXDQ_LORA_W2) return MIXDQ_ERR_SHAPE;
  if (L.mode < 0 || L.mode > MIXDQ_LORA_W2 || (L.rule != MIXDQ_LORA_KEEP && L.rule != MIXDQ_LORA_ABSMAX))
    return MIXDQ_ERR_INVALID_ARG;
  // (INT8 storage may hold a narrower quantizer's integers: q|k|v groups widened to one storage kind)
  if (L.mode == MIXDQ_LORA_INT8 && L.bits != 8 && L.bits != 4 && L.bits != 2) return MIXDQ_ERR_INVALID_ARG;
  if (L.mode == MIXDQ_LORA_W4 && L.bits != 4 && L.bits != 2) return MIXDQ_ERR_INVALID_ARG;
  if (L.mode != MIXDQ_LORA_F16 && (!L.weight_scales || !L.scale || !L.act_scale || !L.act_zero_point))
    return MIXDQ_ERR_INVALID_ARG;
  if (L.R % 32 != 0 || L.R < 32 || L.R > 256 || L.Kf % 4 != 0) return MIXDQ_ERR_SHAPE;
  if (L.mode == MIXDQ_LORA_W4 && L.Kf % 32 != 0) return MIXDQ_ERR_SHAPE;
  if (L.tap_len < 4 || L.tap_len % 4 != 0 || L.Kf % L.tap_len != 0 || L.Kf / L.tap_len > kMaxTaps) return MIXDQ_ERR_SHAPE;
  if (L.ldw % 4 != 0 || L.w_col0 % 4 != 0 || L.w_col0 < 0 || L.ldw < 0) return MIXDQ_ERR_SHAPE;
  if (!aligned(L.W, 8) || !aligned(L.Bcat, 8) || !aligned(L.Acat, 8) || !aligned(L.svec, 16) || !aligned(L.out, 16))
    return MIXDQ_ERR_SHAPE;
  if (!aligned(L.row_map, 4) || !aligned(L.weight_scales, 4) || !aligned(L.wsum, 4) || !aligned(L.bias0, 4) ||
      !aligned(L.scale, 4) || !aligned(L.act_scale, 4) || !aligned(L.act_zero_point, 4))
    return MIXDQ_ERR_SHAPE;
  return MIXDQ_OK;
}

}  // namespace
}  // namespace mixdq

extern "C" int mixdq_lora_table(const mixdq_lora_layer* layers, int n_layers, int32_t* order, int32_t* prefix) {
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

extern "C" int mixdq_lora_status(const mixdq_lora_layer* layers_host, int n_layers) {
  if (!layers_host || n_layers < 1) return MIXDQ_ERR_INVALID_ARG;
  for (int i = 0; i < n_layers; ++i) {
    const int st = mixdq::layer_status(layers_host[i]);
    if (st != MIXDQ_OK) return st;
  }
  return MIXDQ_OK;
}

extern "C" int mixdq_lora_requant(const mixdq_lora_layer* layers_host, const mixdq_lora_layer* layers_device,
                                  const int32_t* prefix_device, int n_layers, mixdq_stream_t stream) {
  using namespace mixdq;
  if (!layers_device || !prefix_device) return MIXDQ_ERR_INVALID_ARG;
  const int st = mixdq_lora_status(layers_host, n_layers);
  if (st != MIXDQ_OK) return st;
  int64_t blocks = 0;
  for (int i = 0; i < n_layers; ++i) blocks += (layers_host[i].N + kRows - 1) / kRows;
  if (blocks > 0x7fffffff || !aligned(layers_device, 8) || !aligned(prefix_device, 4)) return MIXDQ_ERR_INVALID_ARG;
  hipLaunchKernelGGL(lora_requant_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, layers_device,
                     prefix_device, n_layers);
  return launch_status();
}
