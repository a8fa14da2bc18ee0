// The small kernels of the host paths, each behind its launch statement: the row softmax (declared in conv_stack.hip.h), the cache
// remap of zero-padded models and the gather / scatter of a grouped forward_streams (model.h).
#include <algorithm>

#include "model.h"

namespace wekws {

// Row softmax over the last axis (KWSModel.forward_softmax, kws_model.py:89): one wave per row, two passes over the
// row -- online (max, rescaled sum) with 16-byte loads through a 4-byte-aligned type (rows of an odd-width matrix are
// only dword aligned), then normalise in place.  Non-finite logits as torch.softmax has them: a class masked with -Inf
// adds nothing and gets 0; a NaN or +Inf anywhere, or -Inf everywhere, makes the whole row NaN.
static __device__ __forceinline__ void softmax_row(float* p, int K, int lane) {
  struct __attribute__((packed, aligned(4))) V4 { float v[4]; };
  const int K4 = K & ~3;
  float mx = -INFINITY, s = 0.f;
  auto take = [&](float v) __attribute__((always_inline)) {
    if (v == -INFINITY) return;                              // a masked class adds 0 (mx - v would be Inf - Inf while mx is -Inf)
    if (v > mx) { s *= __expf(mx - v); mx = v; }
    s += __expf(v - mx);
  };
  for (int k = lane * 4; k < K4; k += 256) {
    const V4 q = *reinterpret_cast<const V4*>(p + k);
#pragma unroll
    for (int j = 0; j < 4; ++j) take(q.v[j]);
  }
  if (K4 + lane < K) take(p[K4 + lane]);
  float gm = mx;
  for (int off = 32; off > 0; off >>= 1) gm = fmaxf(gm, __shfl_xor(gm, off));
  // (a lane without a finite class keeps mx = -Inf: its s is 0, or NaN if it saw a NaN, and goes in as it is)
  float gs = (mx == -INFINITY) ? s : s * __expf(mx - gm);
  for (int off = 32; off > 0; off >>= 1) gs += __shfl_xor(gs, off);
  const float inv = 1.0f / gs;
  for (int k = lane * 4; k < K4; k += 256) {
    V4 q = *reinterpret_cast<const V4*>(p + k);
#pragma unroll
    for (int j = 0; j < 4; ++j) q.v[j] = __expf(q.v[j] - gm) * inv;
    *reinterpret_cast<V4*>(p + k) = q;
  }
  if (K4 + lane < K) p[K4 + lane] = __expf(p[K4 + lane] - gm) * inv;
}
static __global__ void softmax_rows_kernel(float* y, int64_t rows, int K) {
  const int64_t row = int64_t(blockIdx.x) * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  softmax_row(y + row * K, K, threadIdx.x & 63);
}
// The same rows of a table-driven call: workgroup (w, i) takes rows 4 i .. 4 i + 3 of table row w, of its yrows.
static __global__ void softmax_stream_rows_kernel(const StreamRow* rows, int K) {
  const StreamRow r = rows[blockIdx.x];
  const int t = int(blockIdx.y) * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (t >= r.yrows) return;
  softmax_row(r.y + int64_t(t) * K, K, threadIdx.x & 63);
}
bool launch_softmax_stream_rows(const StreamRow* rows, int nrows, int max_yrows, int K, hipStream_t stream) {
  hipLaunchKernelGGL(softmax_stream_rows_kernel, dim3(unsigned(nrows), unsigned((max_yrows + 3) / 4)), dim3(256), 0, stream, rows, K);
  return hipGetLastError() == hipSuccess;
}
// the one launch statement of softmax_rows_kernel: four rows (waves) per workgroup
bool launch_softmax_rows(float* y, int64_t rows, int K, hipStream_t stream) {
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(unsigned((rows + 3) / 4)), dim3(256), 0, stream, y, rows, K);
  return hipGetLastError() == hipSuccess;
}

}  // namespace wekws

// (CacheMap: model.h)
static __global__ void cache_remap_kernel(float* __restrict__ dst, const float* __restrict__ src, int B, int Cd, int Pd, int Cs, int Ps,
                                          const CacheMap m) {
  const int64_t n = int64_t(B) * Cd * Pd;
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < n; e += int64_t(gridDim.x) * blockDim.x) {
    const int p = int(e % Pd);
    const int64_t bc = e / Pd;
    const int c = int(bc % Cd), b = int(bc / Cd);
    float v = 0.f;
    if (c < Cs) {
      for (int i = 0; i < m.nb; ++i)
        if (p >= m.d_off[i] && p < m.d_off[i] + m.len[i]) v = src[(int64_t(b) * Cs + c) * Ps + m.s_off[i] + (p - m.d_off[i])];
    }
    dst[e] = v;
  }
}
void remap_cache(float* dst, const float* src, int B, int Cd, int Pd, int Cs, int Ps, const CacheMap& map, hipStream_t stream) {
  const int grid = int(std::min<size_t>((size_t(B) * Cd * Pd + 255) / 256, 4096));
  hipLaunchKernelGGL(cache_remap_kernel, dim3(grid), dim3(256), 0, stream, dst, src, B, Cd, Pd, Cs, Ps, map);
}

// Grouped path: the rows of a bucket out of their places -- features (nb, xrow) and live planes in the forward's cache geometry
// ((outer, nb, inner): GRU (L, nb, H), every other backbone (1, nb, E)) -- and back: outputs (nb, yrow) into the rows of y, the new
// caches into the streams' other planes.
static __global__ void pool_gather_kernel(const wekws::StreamRow* __restrict__ rows, int nb, float* __restrict__ xg, int xrow,
                                          float* __restrict__ cg, int outer, int inner) {
  const wekws::StreamRow r = rows[blockIdx.x];
  const int b = blockIdx.x, step = gridDim.y * blockDim.x, e0 = blockIdx.y * blockDim.x + threadIdx.x;
  for (int e = e0; e < xrow; e += step) xg[int64_t(b) * xrow + e] = r.x[e];
  for (int e = e0; e < outer * inner; e += step) {
    const int o = e / inner, i = e - o * inner;
    cg[(int64_t(o) * nb + b) * inner + i] = r.in_cache[e];
  }
}
static __global__ void pool_scatter_kernel(const wekws::StreamRow* __restrict__ rows, int nb, const float* __restrict__ yg, int yrow,
                                           const float* __restrict__ cg, int outer, int inner) {
  const wekws::StreamRow r = rows[blockIdx.x];
  const int b = blockIdx.x, step = gridDim.y * blockDim.x, e0 = blockIdx.y * blockDim.x + threadIdx.x;
  for (int e = e0; e < yrow; e += step) r.y[e] = yg[int64_t(b) * yrow + e];
  for (int e = e0; e < outer * inner; e += step) {
    const int o = e / inner, i = e - o * inner;
    r.out_cache[e] = cg[(int64_t(o) * nb + b) * inner + i];
  }
}
bool launch_pool_gather(dim3 grid, const wekws::StreamRow* rows, int nb, float* xg, int xrow, float* cg, int outer, int inner,
                        hipStream_t stream) {
  hipLaunchKernelGGL(pool_gather_kernel, grid, dim3(256), 0, stream, rows, nb, xg, xrow, cg, outer, inner);
  return hipGetLastError() == hipSuccess;
}
bool launch_pool_scatter(dim3 grid, const wekws::StreamRow* rows, int nb, const float* yg, int yrow, const float* cg, int outer,
                         int inner, hipStream_t stream) {
  hipLaunchKernelGGL(pool_scatter_kernel, grid, dim3(256), 0, stream, rows, nb, yg, yrow, cg, outer, inner);
  return hipGetLastError() == hipSuccess;
}
