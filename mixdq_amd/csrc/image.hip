// Separable resampling for gfx950: resize, Gaussian mask blur and the crop workflow's feathered paste are one filter
// kernel over host-made tables (mixdq_amd/image.py), with two output stages.  No reference counterpart.
//
//   mixdq_resample            [B, C <= 4, Hs, Ws] uint8 / FP16 / FP32 at any element strides -> dense [B, Hd, Wd, C]
//                             uint8 (pixel scale, or a [-1, 1] source through mixdq_to_uint8) or FP32
//   mixdq_resample_paste_u8   FP16 decode [B, 3, Hm, Wm] -> resized into a per-image window of the full-size uint8
//                             original, blended in place under a binary or soft mask
//   mixdq_mask_bbox           the bounding box of a mask's set pixels, one workgroup per image
//   mixdq_mask_dilate_u8      a mask grown by r pixels (a (2r + 1)^2 square maximum of its binarisation), rows then columns
//
// Arithmetic: include/mixdq_math.h (mixdq_resample_tap: explicit FMAs in tap order, zero weights skipped; the
// horizontal chain of each source row first, then the vertical chain of those FP32 values).
//
// The kernel streams: a workgroup is one wave and covers 64 output columns x 8 output rows.  A
// lane owns one output column (all C channels) of those 8 rows and walks the source rows those 8 windows span
// ONCE, in increasing order: it computes the horizontal value of a source row and adds it into the register
// accumulators of the output rows whose window holds that row -- each output's taps still arrive in tap order, so the
// bits are the specification's.  The row tables and their weights are the same for a whole wave (scalar loads); there
// is no intermediate tensor and no LDS.  Where a table's rows are so far apart that the span is longer than the
// windows together (only a table that resample_table does not make), each output row walks its own window instead:
// the work per wave is bounded by 8 * Ty source rows either way.
#include "common.h"
#include "../../include/mixdq_math.h"

namespace mixdq {
namespace {

constexpr int kTileW = 64;    // output columns of a workgroup: one per lane of a wave
constexpr int kTileH = 8;     // output rows of a wave: the register accumulators
constexpr int kWaves = 1;     // waves (row groups) of a workgroup: one, so that a 512 x 512 output already is 512 workgroups

__device__ __forceinline__ bool px_set(uint8_t u) { return u >= 128; }
__device__ __forceinline__ bool px_set(__half h) { return __half2float(h) >= 0.5f; }
__device__ __forceinline__ bool px_set(float f) { return f >= 0.5f; }

__device__ __forceinline__ float px_value(uint8_t u) { return (float)u; }
__device__ __forceinline__ float px_value(__half h) { return __half2float(h); }
__device__ __forceinline__ float px_value(float f) { return f; }

template <typename T, bool MASK>
__device__ __forceinline__ float px_float(T v) {
  if constexpr (MASK) return px_set(v) ? 255.0f : 0.0f;
  else return px_value(v);
}

// A table start as the kernel uses it: limited to [-T, n - 1].  Every tap of a start below -T reads element 0 and
// every tap of one above n - 1 reads element n - 1, so the limit changes no result -- and start + tap cannot overflow.
__device__ __forceinline__ int sane_start(int s, int T, int n) { return min(max(s, -T), n - 1); }

// The accumulators acc[j][c] of output rows y_base + j (j < ny) of table column x (one lane: its own x; `active`
// lanes only), from the source image src (image b's element (c, y, x) at src + c * sc + y * sh + x * sw).
// xs / wx / ys / wy: image b's tables.  ny, y_base and the row tables are the same in every lane of the wave.
template <typename T, bool MASK>
__device__ __forceinline__ void resample_rows(const T* __restrict__ src, int64_t sc, int64_t sh, int64_t sw, int C, int Hs,
                                              int Ws, const int32_t* __restrict__ xs, const float* __restrict__ wx, int Tx,
                                              const int32_t* __restrict__ ys, const float* __restrict__ wy, int Ty, int x,
                                              int y_base, int ny, bool active, float (&acc)[kTileH][4]) {
#pragma unroll
  for (int j = 0; j < kTileH; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[j][c] = 0.0f;
  int ysr[kTileH];
  int lo = 0x7fffffff, hi = -0x7fffffff;
#pragma unroll
  for (int j = 0; j < kTileH; ++j) {
    ysr[j] = j < ny ? sane_start(ys[y_base + j], Ty, Hs) : 0;
    if (j < ny) {
      lo = min(lo, ysr[j]);
      hi = max(hi, ysr[j] + Ty);
    }
  }
  const int x0 = active ? sane_start(xs[x], Tx, Ws) : 0;
  const float* __restrict__ wrow = wx + (int64_t)x * Tx;
  const bool stream = hi - lo <= ny * Ty;
  const int passes = stream ? 1 : ny;
  for (int pass = 0; pass < passes; ++pass) {
    const int r0 = stream ? lo : sane_start(ys[y_base + pass], Ty, Hs);
    const int r1 = stream ? hi : r0 + Ty;
    for (int rr = r0; rr < r1; ++rr) {
      bool wanted = false;
#pragma unroll
      for (int j = 0; j < kTileH; ++j)
        wanted |= j < ny && (stream || j == pass) && rr >= ysr[j] && rr < ysr[j] + Ty;
      if (!wanted) continue;                                   // (a gap between two windows; wave-uniform)
      float h[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (active) {
        const T* __restrict__ row = src + (int64_t)min(max(rr, 0), Hs - 1) * sh;
        for (int i = 0; i < Tx; ++i) {
          const float w = wrow[i];
          const T* __restrict__ px = row + (int64_t)min(max(x0 + i, 0), Ws - 1) * sw;
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c < C) h[c] = mixdq_resample_tap(h[c], w, px_float<T, MASK>(px[c * sc]));
        }
      }
#pragma unroll
      for (int j = 0; j < kTileH; ++j) {
        const int k = rr - ysr[j];
        if (j < ny && (stream || j == pass) && k >= 0 && k < Ty) {
          const float w = wy[(int64_t)(y_base + j) * Ty + k];
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (c < C) acc[j][c] = mixdq_resample_tap(acc[j][c], w, h[c]);
        }
      }
    }
  }
}

// the wave's row group, as a value the compiler knows to be the same in every lane
__device__ __forceinline__ int wave_row() { return __builtin_amdgcn_readfirstlane((int)threadIdx.y); }

template <typename T, bool MASK>
__global__ __launch_bounds__(kTileW* kWaves) void resample_kernel(const T* __restrict__ src, int64_t sb, int64_t sc,
                                                                  int64_t sh, int64_t sw, void* __restrict__ dst,
                                                                  int dst_kind, const int32_t* __restrict__ xs,
                                                                  const float* __restrict__ wx, int Tx,
                                                                  const int32_t* __restrict__ ys,
                                                                  const float* __restrict__ wy, int Ty, int Bt, int B,
                                                                  int C, int Hs, int Ws, int Hd, int Wd) {
  const int x = (int)blockIdx.x * kTileW + (int)threadIdx.x;
  const int y_base = ((int)blockIdx.y * kWaves + wave_row()) * kTileH;
  if (y_base >= Hd) return;                                    // (the whole wave)
  const int ny = min(kTileH, Hd - y_base);
  const bool active = x < Wd;
  for (int b = (int)blockIdx.z; b < B; b += (int)gridDim.z) {
    const int tb = Bt == 1 ? 0 : b;
    float acc[kTileH][4];
    resample_rows<T, MASK>(src + (int64_t)b * sb, sc, sh, sw, C, Hs, Ws, xs + (int64_t)tb * Wd,
                           wx + (int64_t)tb * Wd * Tx, Tx, ys + (int64_t)tb * Hd, wy + (int64_t)tb * Hd * Ty, Ty, x,
                           y_base, ny, active, acc);
    if (!active) continue;
#pragma unroll
    for (int j = 0; j < kTileH; ++j) {
      if (j >= ny) break;
      const int64_t o = (((int64_t)b * Hd + (y_base + j)) * Wd + x) * C;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c >= C) break;
        if (dst_kind == MIXDQ_RESAMPLE_DST_F32) ((float*)dst)[o + c] = acc[j][c];
        else if (dst_kind == MIXDQ_RESAMPLE_DST_U8) ((uint8_t*)dst)[o + c] = mixdq_round_u8(acc[j][c]);
        else ((uint8_t*)dst)[o + c] = mixdq_to_uint8(acc[j][c]);
      }
    }
  }
}

// M: the mask's element type; SOFT: its bytes are the weights (uint8 only)
template <typename M, bool SOFT>
__global__ __launch_bounds__(kTileW* kWaves) void resample_paste_kernel(
    const __half* __restrict__ dec, int64_t db, int64_t dc, int64_t dh, int64_t dw, int Hm, int Wm, uint8_t* out,
    const M* __restrict__ mask, int64_t mb, int64_t mh, int64_t mw, const int32_t* __restrict__ win,
    const int32_t* __restrict__ xs, const float* __restrict__ wx, int Tx, const int32_t* __restrict__ ys,
    const float* __restrict__ wy, int Ty, int Bt, int Ht, int Wt, int B, int H, int W) {
  const int xr = (int)blockIdx.x * kTileW + (int)threadIdx.x;   // window-relative: the tables' index
  const int y_base = ((int)blockIdx.y * kWaves + wave_row()) * kTileH;
  if (y_base >= Ht) return;
  for (int b = (int)blockIdx.z; b < B; b += (int)gridDim.z) {
    // the window, clipped to the image and to the tables (scalar loads: the same in every lane)
    const int wx0 = win[4 * b], wy0 = win[4 * b + 1], wx1 = win[4 * b + 2], wy1 = win[4 * b + 3];
    const int64_t rows = min((int64_t)wy1 - wy0, (int64_t)Ht), cols = min((int64_t)wx1 - wx0, (int64_t)Wt);
    if (y_base >= rows) continue;
    const int ny = (int)min((int64_t)kTileH, rows - y_base);
    const int64_t xa = (int64_t)wx0 + xr;                        // the lane's column in the image
    const bool active = xr < cols && xa >= 0 && xa < W;
    const int tb = Bt == 1 ? 0 : b;
    float acc[kTileH][4];
    resample_rows<__half, false>(dec + (int64_t)b * db, dc, dh, dw, 3, Hm, Wm, xs + (int64_t)tb * Wt,
                                 wx + (int64_t)tb * Wt * Tx, Tx, ys + (int64_t)tb * Ht, wy + (int64_t)tb * Ht * Ty, Ty, xr,
                                 y_base, ny, active, acc);
    if (!active) continue;
#pragma unroll
    for (int j = 0; j < kTileH; ++j) {
      if (j >= ny) break;
      const int64_t ya = (int64_t)wy0 + y_base + j;
      if (ya < 0 || ya >= H) continue;
      const M mv = mask[(int64_t)b * mb + ya * mh + xa * mw];
      uint32_t m;
      if constexpr (SOFT) m = (uint32_t)mv;
      else m = px_set(mv) ? 255u : 0u;
      uint8_t* q = out + (((int64_t)b * H + ya) * W + xa) * 3;
      const uint8_t o0 = q[0], o1 = q[1], o2 = q[2];
      q[0] = mixdq_blend_u8((uint8_t)m, mixdq_to_uint8(acc[j][0]), o0);
      q[1] = mixdq_blend_u8((uint8_t)m, mixdq_to_uint8(acc[j][1]), o1);
      q[2] = mixdq_blend_u8((uint8_t)m, mixdq_to_uint8(acc[j][2]), o2);
    }
  }
}

constexpr int kBoxLanes = 1024;

// One workgroup per image: every lane folds its share of the pixels, then a tree in LDS.
template <typename T>
__global__ __launch_bounds__(kBoxLanes) void mask_bbox_kernel(const T* __restrict__ mask, int64_t sb, int64_t sh, int64_t sw,
                                                        int32_t* __restrict__ out, int H, int W) {
  __shared__ int red[4][kBoxLanes];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const T* __restrict__ m = mask + (int64_t)b * sb;
  int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = 0, y1 = 0;          // (x1, y1: one past the largest, 0 while none is set)
  for (int y = 0; y < H; ++y)
#pragma unroll 4
    for (int x = tid; x < W; x += kBoxLanes)
      if (px_set(m[(int64_t)y * sh + (int64_t)x * sw])) {
        x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x + 1); y1 = max(y1, y + 1);
      }
  red[0][tid] = x0; red[1][tid] = y0; red[2][tid] = x1; red[3][tid] = y1;
  __syncthreads();
  for (int s = kBoxLanes / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] = min(red[0][tid], red[0][tid + s]);
      red[1][tid] = min(red[1][tid], red[1][tid + s]);
      red[2][tid] = max(red[2][tid], red[2][tid + s]);
      red[3][tid] = max(red[3][tid], red[3][tid + s]);
    }
    __syncthreads();
  }
  if (tid < 4) {
    const bool none = red[2][0] == 0;
    out[4 * b + tid] = none ? 0 : red[tid][0];
  }
}

// Mask growth, the rows: one lane = one pixel; tmp = 255 where any pixel of columns x - r .. x + r of its own row is set.
// The window is clipped to the row, so nothing is read outside the image; neighbouring lanes read neighbouring bytes.
template <typename T>
__global__ __launch_bounds__(256) void mask_dilate_rows_kernel(const T* __restrict__ mask, int64_t sb, int64_t sh,
                                                               int64_t sw, uint8_t* __restrict__ tmp, int64_t pixels, int H,
                                                               int W, int r) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += stride) {
    const int64_t row = i / W;
    const int x = (int)(i - row * W);
    const int64_t b = row / H;
    const int y = (int)(row - b * H);
    const T* __restrict__ p = mask + (b * sb + (int64_t)y * sh);
    const int x0 = max(x - r, 0), x1 = min(x + r, W - 1);
    bool set = false;
    for (int k = x0; k <= x1; ++k) set |= px_set(p[(int64_t)k * sw]);
    tmp[i] = set ? 255 : 0;
  }
}

// ... and the columns: out = 255 where any tmp of rows y - r .. y + r of the same image and column is non-zero.  The
// window is clipped to the image's own rows: it never reaches the neighbouring image of the batch.
__global__ __launch_bounds__(256) void mask_dilate_cols_kernel(const uint8_t* __restrict__ tmp, uint8_t* __restrict__ out,
                                                               int64_t pixels, int H, int W, int r) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += stride) {
    const int64_t row = i / W;
    const int x = (int)(i - row * W);
    const int64_t b = row / H;
    const int y = (int)(row - b * H);
    const uint8_t* __restrict__ p = tmp + (b * H * (int64_t)W + x);
    const int y0 = max(y - r, 0), y1 = min(y + r, H - 1);
    uint32_t any = 0;
    for (int k = y0; k <= y1; ++k) any |= p[(int64_t)k * W];
    out[i] = any ? 255 : 0;
  }
}

bool taps_ok(int T) { return T >= 1 && T <= MIXDQ_RESAMPLE_MAX_TAPS; }

dim3 tile_grid(int Hd, int Wd, int B) {
  return dim3((unsigned)((Wd + kTileW - 1) / kTileW), (unsigned)((Hd + kTileH * kWaves - 1) / (kTileH * kWaves)),
              (unsigned)(B < 65535 ? B : 65535));
}

}  // namespace
}  // namespace mixdq

using namespace mixdq;

extern "C" int mixdq_resample(const void* src, int dtype, int64_t sb, int64_t sc, int64_t sh, int64_t sw, int src_mode,
                              void* dst, int dst_kind, const int32_t* xs, const float* wx, int Tx, const int32_t* ys,
                              const float* wy, int Ty, int Bt, int B, int C, int Hs, int Ws, int Hd, int Wd,
                              mixdq_stream_t stream_) {
  const int elem = image_elem_size(dtype);
  if (B < 0 || Hs < 0 || Ws < 0 || Hd < 0 || Wd < 0 || C < 1 || C > 4 || !elem) return MIXDQ_ERR_INVALID_ARG;
  if (src_mode != MIXDQ_RESAMPLE_SRC_VALUE && src_mode != MIXDQ_RESAMPLE_SRC_MASK) return MIXDQ_ERR_INVALID_ARG;
  if (dst_kind != MIXDQ_RESAMPLE_DST_U8 && dst_kind != MIXDQ_RESAMPLE_DST_U8_UNIT && dst_kind != MIXDQ_RESAMPLE_DST_F32)
    return MIXDQ_ERR_INVALID_ARG;
  if (!taps_ok(Tx) || !taps_ok(Ty) || (Bt != 1 && Bt != B)) return MIXDQ_ERR_INVALID_ARG;
  if ((int64_t)B * Hd * Wd == 0) return MIXDQ_OK;    // (an empty tensor has no storage: before the pointer checks)
  if ((int64_t)Hs * Ws == 0) return MIXDQ_ERR_INVALID_ARG;
  if (Hd > 65535 * kTileH * kWaves) return MIXDQ_ERR_INVALID_ARG;
  if (!src || !dst || !xs || !wx || !ys || !wy) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)src % elem || (dst_kind == MIXDQ_RESAMPLE_DST_F32 && (uintptr_t)dst % 4) || (uintptr_t)xs % 4 ||
      (uintptr_t)wx % 4 || (uintptr_t)ys % 4 || (uintptr_t)wy % 4)
    return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid = tile_grid(Hd, Wd, B), block(kTileW, kWaves);
  const bool mask = src_mode == MIXDQ_RESAMPLE_SRC_MASK;
  with_image_type(dtype, [&](auto t) {
    with_bool(mask, [&](auto m) {
      using T = decltype(t);
      resample_kernel<T, decltype(m)::value><<<grid, block, 0, stream>>>(
          (const T*)src, sb, sc, sh, sw, dst, dst_kind, xs, wx, Tx, ys, wy, Ty, Bt, B, C, Hs, Ws, Hd, Wd);
    });
  });
  return launch_status();
}

extern "C" int mixdq_resample_paste_u8(const void* decoded_f16, int64_t db, int64_t dc, int64_t dh, int64_t dw, int Hm,
                                       int Wm, uint8_t* out, const void* mask, int mask_dtype, int64_t mb, int64_t mh,
                                       int64_t mw, int mask_mode, const int32_t* win, const int32_t* xs, const float* wx,
                                       int Tx, const int32_t* ys, const float* wy, int Ty, int Bt, int Ht, int Wt, int B,
                                       int H, int W, mixdq_stream_t stream_) {
  const int elem = image_elem_size(mask_dtype);
  if (B < 0 || H < 0 || W < 0 || Hm < 0 || Wm < 0 || Ht < 0 || Wt < 0 || !elem) return MIXDQ_ERR_INVALID_ARG;
  if (mask_mode != MIXDQ_PASTE_MASK_BINARY && mask_mode != MIXDQ_PASTE_MASK_SOFT) return MIXDQ_ERR_INVALID_ARG;
  if (mask_mode == MIXDQ_PASTE_MASK_SOFT && mask_dtype != MIXDQ_IMAGE_U8) return MIXDQ_ERR_INVALID_ARG;
  if (!taps_ok(Tx) || !taps_ok(Ty) || (Bt != 1 && Bt != B)) return MIXDQ_ERR_INVALID_ARG;
  if ((int64_t)B * Ht * Wt == 0 || (int64_t)B * H * W == 0) return MIXDQ_OK;     // (before the pointer checks)
  if ((int64_t)Hm * Wm == 0) return MIXDQ_ERR_INVALID_ARG;
  if (Ht > 65535 * kTileH * kWaves) return MIXDQ_ERR_INVALID_ARG;
  if (!decoded_f16 || !out || !mask || !win || !xs || !wx || !ys || !wy) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)decoded_f16 % 2 || (uintptr_t)mask % elem || (uintptr_t)win % 4 || (uintptr_t)xs % 4 ||
      (uintptr_t)wx % 4 || (uintptr_t)ys % 4 || (uintptr_t)wy % 4)
    return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid = tile_grid(Ht, Wt, B), block(kTileW, kWaves);
  const __half* d = (const __half*)decoded_f16;
  with_image_type(mask_dtype, [&](auto t) {
    with_bool(mask_mode == MIXDQ_PASTE_MASK_SOFT, [&](auto soft) {
      using M = decltype(t);
      constexpr bool S = decltype(soft)::value;
      if constexpr (!S || std::is_same_v<M, uint8_t>)   // a soft mask is uint8 (checked above)
        resample_paste_kernel<M, S><<<grid, block, 0, stream>>>(d, db, dc, dh, dw, Hm, Wm, out, (const M*)mask, mb, mh,
                                                                mw, win, xs, wx, Tx, ys, wy, Ty, Bt, Ht, Wt, B, H, W);
    });
  });
  return launch_status();
}

extern "C" int mixdq_mask_bbox(const void* mask, int dtype, int64_t sb, int64_t sh, int64_t sw, int32_t* out, int B, int H,
                               int W, mixdq_stream_t stream_) {
  const int elem = image_elem_size(dtype);
  if (B < 0 || H < 0 || W < 0 || !elem) return MIXDQ_ERR_INVALID_ARG;
  if ((int64_t)B * H * W == 0) return MIXDQ_OK;      // (an empty tensor has no storage: before the pointer checks)
  if (!mask || !out) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)mask % elem || (uintptr_t)out % 4) return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  with_image_type(dtype, [&](auto t) {
    using T = decltype(t);
    mask_bbox_kernel<T><<<B, kBoxLanes, 0, stream>>>((const T*)mask, sb, sh, sw, out, H, W);
  });
  return launch_status();
}

extern "C" int mixdq_mask_dilate_u8(const void* mask, int dtype, int64_t sb, int64_t sh, int64_t sw, uint8_t* scratch,
                                    uint8_t* out, int B, int H, int W, int radius, mixdq_stream_t stream_) {
  const int elem = image_elem_size(dtype);
  if (B < 0 || H < 0 || W < 0 || !elem || radius < 0 || radius > 255) return MIXDQ_ERR_INVALID_ARG;
  const int64_t pixels = (int64_t)B * H * W;
  if (pixels == 0) return MIXDQ_OK;                  // (an empty tensor has no storage: before the pointer checks)
  if (!mask || !scratch || !out || scratch == out) return MIXDQ_ERR_INVALID_ARG;
  if ((uintptr_t)mask % elem) return MIXDQ_ERR_ALIGNMENT;
  hipStream_t stream = (hipStream_t)stream_;
  const int blocks = grid_blocks(pixels, 32);
  with_image_type(dtype, [&](auto t) {
    using T = decltype(t);
    mask_dilate_rows_kernel<T><<<blocks, 256, 0, stream>>>((const T*)mask, sb, sh, sw, scratch, pixels, H, W, radius);
  });
  if (launch_status() != MIXDQ_OK) return MIXDQ_ERR_LAUNCH;
  mask_dilate_cols_kernel<<<blocks, 256, 0, stream>>>(scratch, out, pixels, H, W, radius);
  return launch_status();
}
