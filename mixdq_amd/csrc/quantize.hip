// a1: FP16 -> INT8 per-tensor affine quantize for gfx950.
// Replaces quantize_kernel.cu:10-48 and quantize_kernel_vectorized.cu:29-95 of the reference
// (one kernel family serves both exported names).
//
// HBM-bound: 2 B read + 1 B written per element.  Dense path: each lane moves 16 B in / 8 B out
// per step, grid-stride, 4 independent loads in flight per lane.  Strided path: dims are sorted
// by input stride and collapsed on the host; the innermost run is vectorised when it is
// contiguous on both sides and 16-B / 8-B aligned.
#include "common.h"

namespace mixdq {
namespace {

template <bool UNFUSED, bool A4>
__device__ __forceinline__ Char8 quantize8(const Half8& h, float s_inv, float zp) {
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = half_at(h, j);
  const uint2 q = quantize_pack8<UNFUSED, A4>(x, s_inv, zp);     // common.h: clamp + packing by v_ashr_pk_i8_i32 / v_perm_b32
  Char8 out;
  out.w[0] = q.x;
  out.w[1] = q.y;
  return out;
}

template <bool UNFUSED, bool A4>
__device__ __forceinline__ int8_t quantize1(const __half* p, float s_inv, float zp) {
  return (int8_t)quantize_one<UNFUSED, A4>(__half2float(*p), s_inv, zp);
}

// Dense: x and out are linear over numel elements.
template <bool UNFUSED, bool A4 = false>
__global__ __launch_bounds__(256) void quantize_dense_kernel(const __half* __restrict__ x,
                                                             int8_t* __restrict__ out,
                                                             const float* __restrict__ s_inv_p,
                                                             const float* __restrict__ zp_p,
                                                             int64_t numel) {
  const float s_inv = *s_inv_p;
  const float zp = *zp_p;
  const int64_t nvec = numel >> 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const Half8* xv = reinterpret_cast<const Half8*>(x);
  Char8* ov = reinterpret_cast<Char8*>(out);
  // 4 independent 16-B loads in flight per lane
  for (; i + 3 * stride < nvec; i += 4 * stride) {
    Half8 a = xv[i], b = xv[i + stride], c = xv[i + 2 * stride], d = xv[i + 3 * stride];
    ov[i] = quantize8<UNFUSED, A4>(a, s_inv, zp);
    ov[i + stride] = quantize8<UNFUSED, A4>(b, s_inv, zp);
    ov[i + 2 * stride] = quantize8<UNFUSED, A4>(c, s_inv, zp);
    ov[i + 3 * stride] = quantize8<UNFUSED, A4>(d, s_inv, zp);
  }
  for (; i < nvec; i += stride) ov[i] = quantize8<UNFUSED, A4>(xv[i], s_inv, zp);
  // tail (numel % 8 elements), by the first threads of block 0
  const int64_t tail0 = nvec << 3;
  if (blockIdx.x == 0 && threadIdx.x < (numel - tail0)) {
    out[tail0 + threadIdx.x] = quantize1<UNFUSED, A4>(x + tail0 + threadIdx.x, s_inv, zp);
  }
}

struct StridedArgs {
  int64_t size[4];      // collapsed logical sizes, slowest first; size[3] = inner
  int64_t xs[4];        // x strides (elements)
  int64_t os[4];        // out strides (elements)
};

// Strided, inner dimension contiguous on both sides and vectorisable by 8.
template <bool UNFUSED, bool A4 = false>
__global__ __launch_bounds__(256) void quantize_rows_kernel(const __half* __restrict__ x,
                                                            int8_t* __restrict__ out,
                                                            const float* __restrict__ s_inv_p,
                                                            const float* __restrict__ zp_p,
                                                            StridedArgs a) {
  const float s_inv = *s_inv_p;
  const float zp = *zp_p;
  const int64_t inner8 = a.size[3] >> 3;
  const int64_t total = a.size[0] * a.size[1] * a.size[2] * inner8;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    int64_t v = t % inner8;
    int64_t r = t / inner8;
    int64_t i2 = r % a.size[2];
    r /= a.size[2];
    int64_t i1 = r % a.size[1];
    int64_t i0 = r / a.size[1];
    const __half* xp = x + i0 * a.xs[0] + i1 * a.xs[1] + i2 * a.xs[2] + v * 8;
    int8_t* op = out + i0 * a.os[0] + i1 * a.os[1] + i2 * a.os[2] + v * 8;
    *reinterpret_cast<Char8*>(op) =
        quantize8<UNFUSED, A4>(*reinterpret_cast<const Half8*>(xp), s_inv, zp);
  }
}

// Fully general: one element per thread-step.
template <bool UNFUSED, bool A4 = false>
__global__ __launch_bounds__(256) void quantize_scalar_kernel(const __half* __restrict__ x,
                                                              int8_t* __restrict__ out,
                                                              const float* __restrict__ s_inv_p,
                                                              const float* __restrict__ zp_p,
                                                              StridedArgs a) {
  const float s_inv = *s_inv_p;
  const float zp = *zp_p;
  const int64_t total = a.size[0] * a.size[1] * a.size[2] * a.size[3];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    int64_t i3 = t % a.size[3];
    int64_t r = t / a.size[3];
    int64_t i2 = r % a.size[2];
    r /= a.size[2];
    int64_t i1 = r % a.size[1];
    int64_t i0 = r / a.size[1];
    out[i0 * a.os[0] + i1 * a.os[1] + i2 * a.os[2] + i3 * a.os[3]] = quantize1<UNFUSED, A4>(
        x + i0 * a.xs[0] + i1 * a.xs[1] + i2 * a.xs[2] + i3 * a.xs[3], s_inv, zp);
  }
}

// Token + position embedding (mixdq_embed_tokens_f16): one 16-byte chunk of an output row per thread-step,
// out = f16(f32(tok[id]) + f32(pos[t])) -- torch's half add.  An id outside [0, V) is clamped: the kernel has no
// way to report it.
__global__ __launch_bounds__(256) void embed_tokens_kernel(const int* __restrict__ ids, const uint4* __restrict__ tok,
                                                           const uint4* __restrict__ pos, uint4* __restrict__ out,
                                                           int64_t chunks, int T, int cpr, int V) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += stride) {
    const int64_t row = i / cpr;
    const int ch = (int)(i - row * cpr);
    const int t = (int)(row % T);
    const int id = min(max(ids[row], 0), V - 1);
    const uint4 a = tok[(int64_t)id * cpr + ch], b = pos[(int64_t)t * cpr + ch];
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const v2h ah = *reinterpret_cast<const v2h*>(&aw[e]), bh = *reinterpret_cast<const v2h*>(&bw[e]);
      v2f r = __builtin_convertvector(ah, v2f) + __builtin_convertvector(bh, v2f);
      asm("" : "+v"(r));
      const v2h h = __builtin_convertvector(r, v2h);
      o[e] = *reinterpret_cast<const uint32_t*>(&h);
    }
    out[i] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// What one mixdq_quantize_f16_i8 call launches: the planner's answer (mixdq_quantize_f16_i8_route reports it).
enum { kRouteNone = -1, kRouteDense = 0, kRouteRows = 1, kRouteScalar = 2 };
struct QuantizePlan {
  int route;            // kRouteNone: no element, nothing is launched
  int rank;             // dimensions left after the sort and the collapse (m; 0 with kRouteNone)
  int blocks;           // grid of the launch (256 lanes a block)
  int64_t numel;
  StridedArgs a;        // the collapsed dimensions, right-aligned (dense: size[3] = numel)
};

// Sort the dimensions by x stride (descending), drop size-1 dimensions, collapse mergeable neighbours, and choose
// the kernel and its grid.  Host arithmetic only: x and out are looked at for their alignment, never dereferenced.
inline int plan_quantize(const int64_t* sizes, const int64_t* x_strides, const int64_t* out_strides, int ndim,
                         const void* x, const void* out, QuantizePlan* p) {
  int64_t sz[8], xs[8], os[8];
  int n = 0;
  int64_t numel = 1;
  for (int d = 0; d < ndim; ++d) {
    if (sizes[d] < 0 || x_strides[d] < 0 || out_strides[d] < 0) return MIXDQ_ERR_INVALID_ARG;
    numel *= sizes[d];
    if (sizes[d] != 1) {
      sz[n] = sizes[d]; xs[n] = x_strides[d]; os[n] = out_strides[d]; ++n;
    }
  }
  p->route = kRouteNone; p->rank = 0; p->blocks = 0; p->numel = numel;
  for (int i = 0; i < 4; ++i) { p->a.size[i] = 1; p->a.xs[i] = 0; p->a.os[i] = 0; }
  if (numel == 0) { p->a.size[3] = 0; return MIXDQ_OK; }
  if (!x || !out) return MIXDQ_ERR_INVALID_ARG;
  for (int i = 1; i < n; ++i)   // insertion sort, stable
    for (int j = i; j > 0 && xs[j - 1] < xs[j]; --j) {
      int64_t t;
      t = sz[j]; sz[j] = sz[j - 1]; sz[j - 1] = t;
      t = xs[j]; xs[j] = xs[j - 1]; xs[j - 1] = t;
      t = os[j]; os[j] = os[j - 1]; os[j - 1] = t;
    }
  int m = 0;
  for (int i = 0; i < n; ++i) {
    if (m > 0 && xs[m - 1] == xs[i] * sz[i] && os[m - 1] == os[i] * sz[i]) {
      sz[m - 1] *= sz[i]; xs[m - 1] = xs[i]; os[m - 1] = os[i];
    } else {
      sz[m] = sz[i]; xs[m] = xs[i]; os[m] = os[i]; ++m;
    }
  }
  if (m == 0) { sz[0] = 1; xs[0] = 1; os[0] = 1; m = 1; }
  if (m > 4) return MIXDQ_ERR_SHAPE;
  StridedArgs& a = p->a;
  for (int i = 0; i < m; ++i) {
    a.size[4 - m + i] = sz[i]; a.xs[4 - m + i] = xs[i]; a.os[4 - m + i] = os[i];
  }
  p->rank = m;
  const bool aligned = ((uintptr_t)x % 16 == 0) && ((uintptr_t)out % 8 == 0);
  if (m == 1 && xs[0] == 1 && os[0] == 1 && aligned) {
    p->route = kRouteDense;
    p->blocks = grid_blocks((numel >> 3) + 1);
    return MIXDQ_OK;
  }
  bool rows_ok = aligned && a.xs[3] == 1 && a.os[3] == 1 && a.size[3] % 8 == 0;
  for (int i = 0; i < 3 && rows_ok; ++i)
    if (a.size[i] > 1 && (a.xs[i] % 8 != 0 || a.os[i] % 8 != 0)) rows_ok = false;
  p->route = rows_ok ? kRouteRows : kRouteScalar;
  p->blocks = grid_blocks(rows_ok ? numel >> 3 : numel);
  return MIXDQ_OK;
}

}  // namespace
}  // namespace mixdq

using namespace mixdq;

extern "C" int mixdq_quantize_f16_i8(const void* x_f16, int8_t* out, const int64_t* sizes,
                                     const int64_t* x_strides, const int64_t* out_strides,
                                     int ndim, const float* scale_inv, const float* zero_point,
                                     int flags, mixdq_stream_t stream_) {
  if (flags & MIXDQ_FLAG_ACT_ANY) return MIXDQ_ERR_UNSUPPORTED;   // mixdq_linear_f16's epilogue activations
  if (ndim < 0 || ndim > 8 || !scale_inv || !zero_point) return MIXDQ_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  if (flags & (MIXDQ_FLAG_A4_1 | MIXDQ_FLAG_A4_2)) return MIXDQ_ERR_UNSUPPORTED;   // one quantizer: slot 0
  const bool unfused = flags & MIXDQ_FLAG_UNFUSED, a4 = flags & MIXDQ_FLAG_A4_0;
  QuantizePlan p;
  const int status = plan_quantize(sizes, x_strides, out_strides, ndim, x_f16, out, &p);
  if (status != MIXDQ_OK || p.route == kRouteNone) return status;
  const __half* x = (const __half*)x_f16;
  const int grid = p.blocks;
  with_bool(unfused, [&](auto u) {
    with_bool(a4, [&](auto a) {
      constexpr bool U = decltype(u)::value, A4 = decltype(a)::value;
      if (p.route == kRouteDense) quantize_dense_kernel<U, A4><<<grid, 256, 0, stream>>>(x, out, scale_inv, zero_point, p.numel);
      else if (p.route == kRouteRows) quantize_rows_kernel<U, A4><<<grid, 256, 0, stream>>>(x, out, scale_inv, zero_point, p.a);
      else quantize_scalar_kernel<U, A4><<<grid, 256, 0, stream>>>(x, out, scale_inv, zero_point, p.a);
    });
  });
  return launch_status();
}

extern "C" int mixdq_quantize_f16_i8_route(const int64_t* sizes, const int64_t* x_strides,
                                           const int64_t* out_strides, int ndim, const void* x_f16,
                                           const void* out, int* route, int* rank,
                                           int64_t* collapsed_sizes4, int* blocks) {
  if (ndim < 0 || ndim > 8) return MIXDQ_ERR_INVALID_ARG;
  QuantizePlan p;
  const int status = plan_quantize(sizes, x_strides, out_strides, ndim, x_f16, out, &p);
  if (status != MIXDQ_OK) return status;
  if (route) *route = p.route;
  if (rank) *rank = p.rank;
  if (blocks) *blocks = p.blocks;
  if (collapsed_sizes4)
    for (int i = 0; i < 4; ++i) collapsed_sizes4[i] = p.a.size[i];
  return MIXDQ_OK;
}

extern "C" int mixdq_embed_tokens_f16(const int32_t* ids, const void* tok_f16, const void* pos_f16, void* out_f16,
                                      int B, int T, int C, int V, mixdq_stream_t stream_) {
  if (B < 0 || T < 0 || C < 0 || V < 1) return MIXDQ_ERR_INVALID_ARG;
  if (C % 8 != 0) return MIXDQ_ERR_ALIGNMENT;
  const int64_t chunks = (int64_t)B * T * (C / 8);
  if (chunks == 0) return MIXDQ_OK;
  if (!ids || !tok_f16 || !pos_f16 || !out_f16) return MIXDQ_ERR_INVALID_ARG;
  if (((uintptr_t)tok_f16 | (uintptr_t)pos_f16 | (uintptr_t)out_f16) & 15 || ((uintptr_t)ids & 3))
    return MIXDQ_ERR_ALIGNMENT;
  embed_tokens_kernel<<<grid_blocks(chunks), 256, 0, (hipStream_t)stream_>>>(
      ids, (const uint4*)tok_f16, (const uint4*)pos_f16, (uint4*)out_f16, chunks, T, C / 8, V);
  return launch_status();
}
