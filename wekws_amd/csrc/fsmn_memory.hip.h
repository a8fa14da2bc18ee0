// The trainable FSMN memory block on the device: the reference's FSMNBlock.forward (wekws/model/fsmn.py:214-253, empty cache)
// and its autograd, as a causal sparse FIR per channel over a (B, T, D) float32 tensor.  fsmn_memory_plan.h has the tap table,
// the tiles and the workspace; three kernels:
//   fsmn_memory_fir_kernel<VEC, BWD>   one workgroup owns kFsmnMemFirTile frames of one row and kFsmnMemChannels channels.  It
//                        copies those frames and the window before (forward) or after (backward) them into LDS once, with the
//                        taps' coefficients beside them, and every lane adds its taps by exact float32 fmaf in the table's
//                        order.  BWD = false: y from x, delays looking back, frames before 0 are arithmetic zeros (an Inf tap
//                        makes the first frames NaN, as the reference's padding does).  BWD = true: dx from g, the same taps
//                        looking ahead, terms past the row's end left out.  VEC = 4: 16-byte accesses (D % 4 == 0, aligned
//                        bases); VEC = 1: scalars; both add the same products in the same order.
//   fsmn_memory_tap_grad_kernel<VEC>   one workgroup owns kFsmnMemGradTile frames of one row and kFsmnMemChannels channels; a
//                        lane owns one channel and up to four taps and adds g * x over the tile's frames in ascending order in
//                        double (the product of two floats is exact there).  One partial per tile, tap and channel goes to the
//                        workspace as (tiles, lorder + rorder, D) doubles.
//   fsmn_memory_fold_kernel            adds the partials of one tap and kFsmnMemChannels channels: up to kFsmnMemFoldSegs
//                        segments of consecutive tiles in ascending order, then the segments' sums in ascending order, rounds
//                        to float32 once and writes grad_w_left / grad_w_right.
// A row's y and dx depend on that row alone; the tap gradient's order of additions is a function of the shape alone.  No
// floating-point atomics; nothing synchronises, allocates or reads on the host.  This object is built with -fno-slp-vectorize
// (DESIGN.md 3.8): the four fmaf of a 16-byte access and the double chains stay scalar instructions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fsmn_memory_plan.h"

namespace wekws {

// what the kernels are told: the shape and, per tap, where its coefficient comes from and which LDS row it reads
struct FsmnMemArgs {
  int T, D, lorder, rorder;
  int ntaps;                                  // 1 + lorder + rorder
  int halo;                                   // window - 1: the largest delay
  int tiles_t;                                // frame tiles of a row (of the kernel that is launched)
  int16_t off[1 + kFsmnMemMaxTaps];           // forward and tap gradient: halo - delay; backward: delay
  uint8_t source[1 + kFsmnMemMaxTaps];
  uint8_t index[1 + kFsmnMemMaxTaps];
};

// lds[r][c] = src[b, frame0 + r, ch0 + c] for r < nrows, c < kFsmnMemChannels; 0 where the frame is outside [0, T) or the
// channel is >= D
template <int VEC>
__device__ inline void fsmn_memory_load_rows(float* __restrict__ lds, const float* __restrict__ src, int64_t row_base /* b T */,
                                             int frame0, int nrows, int ch0, int T, int D) {
  constexpr int kCols = kFsmnMemChannels / VEC;
  for (int i = threadIdx.x; i < nrows * kCols; i += kFsmnMemThreads) {
    const int r = i / kCols, c = (i % kCols) * VEC;
    const int f = frame0 + r, ch = ch0 + c;
    const bool in = f >= 0 && f < T && ch < D;             // VEC == 4: D % 4 == 0, so a column is inside or outside as a whole
    if constexpr (VEC == 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in) v = *reinterpret_cast<const float4*>(src + (row_base + f) * D + ch);
      *reinterpret_cast<float4*>(lds + r * kFsmnMemChannels + c) = v;
    } else {
      lds[r * kFsmnMemChannels + c] = in ? src[(row_base + f) * D + ch] : 0.f;
    }
  }
}

// the coefficient of tap k for channel ch
__device__ inline float fsmn_memory_coef(const FsmnMemArgs& a, int k, int ch, const float* __restrict__ wl, const float* __restrict__ wr) {
  const int s = a.source[k], i = a.index[k];
  if (s == kFsmnMemSkip) return 1.f;
  return s == kFsmnMemLeft ? wl[int64_t(ch) * a.lorder + i] : wr[int64_t(ch) * a.rorder + i];
}

template <int VEC, bool BWD>
__global__ __launch_bounds__(kFsmnMemThreads) void fsmn_memory_fir_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                          const float* __restrict__ wl, const float* __restrict__ wr,
                                                                          FsmnMemArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fsmn_memory_lds[];
  constexpr int kCols = kFsmnMemChannels / VEC;             // lanes along the channels
  constexpr int kRows = kFsmnMemThreads / kCols;            // frames the workgroup computes at a time
  constexpr int kOut = kFsmnMemFirTile / kRows;             // frames a lane computes
  const int nrows = kFsmnMemFirTile + a.halo;
  float* xs = fsmn_memory_lds;                               // [nrows][32]
  float* cs = fsmn_memory_lds + nrows * kFsmnMemChannels;    // [ntaps][32]
  const int b = blockIdx.x / a.tiles_t, t0 = (blockIdx.x % a.tiles_t) * kFsmnMemFirTile;
  const int ch0 = blockIdx.y * kFsmnMemChannels;
  const int64_t row_base = int64_t(b) * a.T;
  fsmn_memory_load_rows<VEC>(xs, in, row_base, BWD ? t0 : t0 - a.halo, nrows, ch0, a.T, a.D);
  for (int i = threadIdx.x; i < a.ntaps * kFsmnMemChannels; i += kFsmnMemThreads) {
    const int k = i / kFsmnMemChannels, ch = ch0 + i % kFsmnMemChannels;
    cs[i] = ch < a.D ? fsmn_memory_coef(a, k, ch, wl, wr) : 0.f;
  }
  __syncthreads();
  const int c = (threadIdx.x % kCols) * VEC, fr = threadIdx.x / kCols;
  float acc[kOut][VEC];
  // the skip term: coefficient 1, the product is the value itself
#pragma unroll
  for (int m = 0; m < kOut; ++m) {
    const int j = fr + m * kRows;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      acc[m][e] = xs[(j + a.off[0]) * kFsmnMemChannels + c + e];
      if (BWD && t0 + j + a.off[0] >= a.T) acc[m][e] = 0.f;  // no such term: the sum starts empty
    }
  }
  for (int k = 1; k < a.ntaps; ++k) {
    const int off = a.off[k];
    float w[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) w[e] = cs[k * kFsmnMemChannels + c + e];
#pragma unroll
    for (int m = 0; m < kOut; ++m) {
      const int j = fr + m * kRows;
      const bool exists = !BWD || t0 + j + off < a.T;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float p = fmaf(w[e], xs[(j + off) * kFsmnMemChannels + c + e], acc[m][e]);
        acc[m][e] = exists ? p : acc[m][e];
      }
    }
  }
  const int ch = ch0 + c;
  if (ch >= a.D) return;
#pragma unroll
  for (int m = 0; m < kOut; ++m) {
    const int t = t0 + fr + m * kRows;
    if (t >= a.T) continue;
    float* o = out + (row_base + t) * a.D + ch;
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(o) = make_float4(acc[m][0], acc[m][1], acc[m][2], acc[m][3]);
    else *o = acc[m][0];
  }
}

constexpr int kFsmnMemTapGroups = kFsmnMemThreads / kFsmnMemChannels;                 // 8: lanes of one channel
constexpr int kFsmnMemTapsPerLane = (kFsmnMemMaxTaps + kFsmnMemTapGroups - 1) / kFsmnMemTapGroups;   // 4

// partial[tile][k][d] = sum over the tile's frames t, ascending, of g[t, d] * x[t - delay_k, d], in double
template <int VEC>
__global__ __launch_bounds__(kFsmnMemThreads) void fsmn_memory_tap_grad_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                               double* __restrict__ partial, FsmnMemArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fsmn_memory_lds[];
  const int xrows = kFsmnMemGradTile + a.halo;
  float* xs = fsmn_memory_lds;                               // [xrows][32]: frames t0 - halo ...
  float* gs = fsmn_memory_lds + xrows * kFsmnMemChannels;    // [kFsmnMemGradTile][32]: frames t0 ...
  const int b = blockIdx.x / a.tiles_t, t0 = (blockIdx.x % a.tiles_t) * kFsmnMemGradTile;
  const int ch0 = blockIdx.y * kFsmnMemChannels;
  const int64_t row_base = int64_t(b) * a.T;
  fsmn_memory_load_rows<VEC>(xs, x, row_base, t0 - a.halo, xrows, ch0, a.T, a.D);
  fsmn_memory_load_rows<VEC>(gs, g, row_base, t0, kFsmnMemGradTile, ch0, a.T, a.D);
  __syncthreads();
  const int c = threadIdx.x % kFsmnMemChannels, q = threadIdx.x / kFsmnMemChannels;
  const int K = a.lorder + a.rorder;
  const int frames = a.T - t0 < kFsmnMemGradTile ? a.T - t0 : kFsmnMemGradTile;       // >= 1; frames past the end do not exist
  int off[kFsmnMemTapsPerLane];
  double acc[kFsmnMemTapsPerLane];
#pragma unroll
  for (int m = 0; m < kFsmnMemTapsPerLane; ++m) {
    off[m] = 0;                                              // (a lane without a tap here adds into a sum nobody stores)
    acc[m] = 0.0;
#pragma unroll
    for (int u = 0; u < kFsmnMemTapGroups; ++u) {            // constant indices into the table: it stays in scalar registers
      const int k = u + m * kFsmnMemTapGroups;
      if (q == u && k < K) off[m] = a.off[1 + k];
    }
  }
  for (int r = 0; r < frames; ++r) {
    const double gv = double(gs[r * kFsmnMemChannels + c]);
#pragma unroll
    for (int m = 0; m < kFsmnMemTapsPerLane; ++m)
      if (m * kFsmnMemTapGroups < K) acc[m] = fma(gv, double(xs[(r + off[m]) * kFsmnMemChannels + c]), acc[m]);   // (uniform)
  }
  const int ch = ch0 + c;
  if (ch >= a.D) return;
#pragma unroll
  for (int m = 0; m < kFsmnMemTapsPerLane; ++m) {
    const int k = q + m * kFsmnMemTapGroups;
    if (k < K) partial[(int64_t(blockIdx.x) * K + k) * a.D + ch] = acc[m];
  }
}

// grid (lorder + rorder, channel blocks): the sums of one tap, rounded to float32 once
__global__ __launch_bounds__(kFsmnMemThreads) void fsmn_memory_fold_kernel(const double* __restrict__ partial, int64_t tiles, int D,
                                                                           int lorder, int rorder, float* __restrict__ dwl,
                                                                           float* __restrict__ dwr) {
  __shared__ double segs[kFsmnMemFoldSegs][kFsmnMemChannels];
  static_assert(kFsmnMemFoldSegs == kFsmnMemTapGroups, "one lane group a segment");
  const int c = threadIdx.x % kFsmnMemChannels, q = threadIdx.x / kFsmnMemChannels;
  const int k = blockIdx.x, K = lorder + rorder;
  const int ch = blockIdx.y * kFsmnMemChannels + c;
  const int64_t len = fsmn_memory_fold_seg_len(tiles);
  const int64_t first = q * len, last = first + len < tiles ? first + len : tiles;
  double s = 0.0;
  if (ch < D)
    for (int64_t t = first; t < last; ++t) s += partial[(t * K + k) * D + ch];
  segs[q][c] = s;
  __syncthreads();
  if (q != 0 || ch >= D) return;
  const int nseg = int((tiles + len - 1) / len);             // segments that hold a tile
  double sum = segs[0][c];
  for (int i = 1; i < nseg; ++i) sum += segs[i][c];
  if (k < lorder) dwl[int64_t(ch) * lorder + k] = float(sum);
  else dwr[int64_t(ch) * rorder + (k - lorder)] = float(sum);
}

}  // namespace wekws
