// Global CMVN statistics on the device: what tools/compute_cmvn_stats.py of the reference accumulates over the training set
// (:26-72 per batch, :128-151 over the batches) -- per bin the sum of the features and the sum of their squares over every
// valid frame, and the frame count -- for (B, T, D) float32 features that are already on the device.
//
// The reference accumulates in float32; these kernels accumulate in double from the first add: (double)x is exact, and so is
// the square of a float32 in double, so each statistic is off the exact sum only by the roundings of the additions.  That is
// the one deviation: a sum the reference's float32 would overflow stays finite here.
//
// Two or three launches a call (cmvn_stats_plan.h has the cut):
//   cmvn_stats_tile_kernel  one workgroup a tile of F consecutive frames (numbered row by row).  Bins across the lanes, G
//                           frames side by side where D leaves room; a lane adds its frames in ascending order, the G lanes
//                           of a bin are folded in lane order through LDS, and the tile's 2 D doubles go to scratch.  A frame
//                           at or past its row's length is skipped by index -- its lane-step adds nothing, so what padding
//                           holds (a NaN, an Inf) cannot reach a sum; a row whose length is outside 0..T is skipped
//                           altogether.  Every load lies inside feats (B, T, D) and lengths (B).
//   cmvn_stats_fold_kernel  per bin the tiles' partials in one fixed order (16 lanes a bin, lane i rows i, i + 16, ..., then
//                           the lanes in order), added to the handle's running sums; a workgroup of its own adds the valid
//                           frames and the rows with a bad length to the handle's two int64 counters.  More than 64 tiles
//                           are first folded 64 at a time by a launch of the same kernel, one workgroup per 64 tiles and
//                           16 bins, so that the fold is spread over the device instead of ceil(D / 16) workgroups.
// So the bits of a call's contribution are a function of (feats, lengths, B, T, D) alone: no floating-point atomics, no
// dependence on the grid or on the CU count.  Non-finite features propagate as IEEE addition has them (no fmax / fmin): a
// NaN gives NaN, +Inf alone +Inf, +Inf and -Inf together NaN in the sums and +Inf in the sums of squares.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cmvn_stats_plan.h"

namespace wekws {

constexpr int kCmvnUnroll = 8;               // loads a lane has in flight

// frames [0, nframes) = B * T; partial: (tiles, 2, D) doubles
__global__ __launch_bounds__(kCmvnThreads) void cmvn_stats_tile_kernel(const float* __restrict__ x, int T, int D,
                                                                       const int32_t* __restrict__ lengths, int nframes,
                                                                       int F, int W, int G, uint32_t tmul, int tshift,
                                                                       double* __restrict__ partial) {
  __shared__ double lds_s[kCmvnThreads], lds_q[kCmvnThreads];
  const int tid = threadIdx.x;
  const int g = tid / W, c0 = tid - g * W;                    // G * W <= 256: lanes past it idle
  const int64_t f0 = int64_t(blockIdx.x) * F;
  const int f1 = int(f0 + F < nframes ? f0 + F : nframes);
  double* out = partial + int64_t(blockIdx.x) * 2 * D;
  for (int cb = 0; cb < D; cb += kCmvnThreads) {              // one trip when D <= 256
    const int c = cb + c0;
    const bool live = g < G && c < D;
    double s = 0.0, q = 0.0;
    if (live) {
      const int64_t first = f0 * D + c;                        // the tile's first frame: where a skipped frame's load is parked
      for (int64_t f = f0 + g; f < f1; f += G * kCmvnUnroll) {  // (64-bit: the last step may pass 2^31)
        // branch-free, so that the loads of a step are in flight together: the rows' lengths, then the features
        int len[kCmvnUnroll], t[kCmvnUnroll];
#pragma unroll
        for (int u = 0; u < kCmvnUnroll; ++u) {
          const int64_t fu = f + u * G;
          const int fc = int(fu < f1 ? fu : f1 - 1);            // past the tile: a frame of the tile, dropped below
          const int b = int((uint64_t(unsigned(fc)) * tmul) >> tshift);   // fc / T (cmvn_div)
          t[u] = fu < f1 ? fc - b * T : T;
          len[u] = lengths ? lengths[b] : T;
        }
        float v[kCmvnUnroll];
        bool ok[kCmvnUnroll];
#pragma unroll
        for (int u = 0; u < kCmvnUnroll; ++u) {
          ok[u] = len[u] >= 0 && len[u] <= T && t[u] < len[u];
          v[u] = x[ok[u] ? (f + u * G) * D + c : first];
        }
#pragma unroll
        for (int u = 0; u < kCmvnUnroll; ++u) {                 // a skipped frame is skipped by index: nothing of it is added
          const double d = double(v[u]);
          const double s1 = s + d, q1 = fma(d, d, q);
          s = ok[u] ? s1 : s;
          q = ok[u] ? q1 : q;
        }
      }
    }
    lds_s[tid] = s;
    lds_q[tid] = q;
    __syncthreads();
    if (live && g == 0) {
      for (int k = 1; k < G; ++k) {
        s += lds_s[k * W + c0];
        q += lds_q[k * W + c0];
      }
      out[c] = s;
      out[D + c] = q;
    }
    __syncthreads();
  }
}

// rows: (nrows, 2, D) doubles.  Workgroup (x, y) folds rows [x seg, min(nrows, (x + 1) seg)) of bins 16 y .. 16 y + 15: lane i of
// a bin rows i, i + 16, ... in turn, then the 16 lanes in order.  counts == NULL: the first stage, out (segments, 2, D) row x is
// written.  Else the last stage (one x, seg >= nrows): out (2, D), the handle's running sums, is added to, and the workgroup
// past the bins adds to counts = {valid frames, rows with a length outside 0..T}.
__global__ __launch_bounds__(kCmvnThreads) void cmvn_stats_fold_kernel(const double* __restrict__ rows, int nrows, int seg, int D,
                                                                       double* __restrict__ out, const int32_t* __restrict__ lengths,
                                                                       int B, int T, int64_t* __restrict__ counts) {
  __shared__ double lds_s[kCmvnThreads], lds_q[kCmvnThreads];
  __shared__ long long lds_n[kCmvnThreads];
  __shared__ int lds_bad[kCmvnThreads];
  const int tid = threadIdx.x;
  if (counts && blockIdx.y == gridDim.y - 1) {                // the counters (integers: any order gives the same)
    long long n = 0;
    int bad = 0;
    for (int b = tid; b < B; b += kCmvnThreads) {
      const int len = lengths ? lengths[b] : T;
      if (len >= 0 && len <= T) n += len;
      else ++bad;
    }
    lds_n[tid] = n;
    lds_bad[tid] = bad;
    __syncthreads();
    for (int off = kCmvnThreads / 2; off > 0; off >>= 1) {
      if (tid < off) { lds_n[tid] += lds_n[tid + off]; lds_bad[tid] += lds_bad[tid + off]; }
      __syncthreads();
    }
    if (tid == 0) { counts[0] += lds_n[0]; counts[1] += lds_bad[0]; }
    return;
  }
  const int lane = tid / kCmvnFoldCols, c = blockIdx.y * kCmvnFoldCols + (tid & (kCmvnFoldCols - 1));
  const int r0 = blockIdx.x * seg, r1 = r0 + seg < nrows ? r0 + seg : nrows;
  double s = 0.0, q = 0.0;
  if (c < D) {
#pragma unroll 4
    for (int i = r0 + lane; i < r1; i += kCmvnFoldLanes) {
      const double* p = rows + int64_t(i) * 2 * D;
      s += p[c];
      q += p[D + c];
    }
  }
  lds_s[tid] = s;
  lds_q[tid] = q;
  __syncthreads();
  if (lane == 0 && c < D) {
    for (int k = 1; k < kCmvnFoldLanes; ++k) {
      s += lds_s[k * kCmvnFoldCols + tid];
      q += lds_q[k * kCmvnFoldCols + tid];
    }
    if (counts) {
      out[c] += s;
      out[D + c] += q;
    } else {
      double* o = out + int64_t(blockIdx.x) * 2 * D;
      o[c] = s;
      o[D + c] = q;
    }
  }
}

}  // namespace wekws
