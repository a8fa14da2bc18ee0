// The trainable BatchNorm1d on the device with the ReLU and the residual add that follow it fused in: the reference's
// DsCnnBlock.cnn[1:3] / [4:6] (wekws/model/tcn.py), DSDilatedConv1d.bn, TCNBlock.bn1 / relu1 and TCNBlock.bn2 + inputs + relu2
// (wekws/model/mdtc.py), and their autograd, over (B, C, T) float32 tensors.  batchnorm_plan.h has the tiles and the workspace.
// Time is the contiguous axis: a row is one (b, c) pair, 32 lanes run along t of one row, a lane owns four consecutive frames
// and a workgroup owns kBnTile frames of kBnRows rows.  Six kernels:
//   batchnorm_stats_kernel<VEC>       per (row, tile): sum d and sum d^2 in double, d = x - shift, shift the channel's first
//                        element x[0, c, 0] (0 when that is not finite): per lane over its frames in ascending order, then the 32
//                        lanes by the butterfly 16, 8, 4, 2, 1.  One pair of partials per (batch row, tile, channel).
//   batchnorm_stats_fold_kernel       per channel: up to kBnFoldSegs segments of consecutive partials in ascending order, then the
//                        segments' sums in ascending order; mean = shift + S1 / N, var = (S2 - S1 S1 / N) / N clamped at 0 by a
//                        comparison a NaN fails, invstd = 1 / sqrt(var + eps), all in double, each rounded to float32 once; the
//                        running buffers and num_batches_tracked are updated here, in double, rounded once.
//   batchnorm_apply_kernel<VEC, RELU, RES, EVAL>   y.  EVAL: the statistics come from the running buffers and the kernel writes
//                        save_mean / save_invstd itself (one launch).
//   batchnorm_grad_sums_kernel<VEC, RELU>   per (row, tile): sum g' and sum g' (x - mean) in double, the same lane order.
//   batchnorm_grad_fold_kernel        per channel, the same fold: grad_bias, grad_weight = invstd sum g' (x - mean), each rounded
//                        once, and the two coefficients of grad_x.
//   batchnorm_grad_x_kernel<VEC, RELU, BATCH>   grad_x and grad_residual.
//
// The float32 operation order, the same in every instance (fmaf is the exact fused operation):
//     a  = weight * invstd                                   (weight absent: invstd)
//     z  = fmaf(x - mean, a, bias)                           (bias absent: +0)
//     z  = z + residual                                      (RES)
//     y  = z < 0 ? 0 : z                                     (RELU; a NaN stays a NaN)
//     g' = y <= 0 ? 0 : grad_y                               (RELU; where y is NaN the gradient passes, as the reference's does)
//     k1 = float(S_g / N),  k2 = float(invstd^2 S_gx / N)    (S_g = sum g', S_gx = sum g' (x - mean), in double)
//     grad_x = fmaf(-(x - mean), k2, g' - k1) * a            (batch statistics)        grad_x = g' * a        (eval)
// VEC = 4: one 16-byte access per lane and tensor (T % 4 == 0, aligned bases); VEC = 1: four scalar accesses of the same
// frames.  VEC changes the copies only: the values, the operations and their order are the same.  A row's y, grad_x and
// grad_residual depend on that row and its channel's statistics alone; the order of every sum is a function of (B, T) alone.  No
// floating-point atomics; nothing synchronises, allocates or reads on the host.  This object is built with -fno-slp-vectorize
// (DESIGN.md 3.8): the float32 chains and the double sums stay scalar instructions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batchnorm_plan.h"

namespace wekws {

static_assert(kBnRowLanes == 32, "a row is half a wave: the butterfly below runs over 32 lanes");
static_assert(kBnLaneFrames == 4, "a lane owns one 16-byte access");

// the shape as the kernels read it
struct BatchNormArgs {
  int64_t rows;                               // B * C
  int C, T;
  int tiles_t;                                // frame tiles of a row
};

// where a lane works: its row (b, c), its first frame; row >= rows: nothing to do
struct BatchNormLane {
  int64_t row, b;
  int c, tile, t, l;
  bool valid;
};

__device__ inline BatchNormLane batchnorm_lane(const BatchNormArgs& a) {
  BatchNormLane p;
  p.tile = int(blockIdx.x % a.tiles_t);
  p.l = threadIdx.x % kBnRowLanes;
  p.row = int64_t(blockIdx.x / a.tiles_t) * kBnRows + threadIdx.x / kBnRowLanes;
  p.valid = p.row < a.rows;
  p.b = p.row / a.C;
  p.c = int(p.row % a.C);
  p.t = p.tile * kBnTile + p.l * kBnLaneFrames;
  return p;
}

// v[j] = row[t + j] for the frames inside [0, T), 0 for the others.  VEC == 4: T % 4 == 0 and t % 4 == 0, so the four frames are
// inside or outside as a whole.
template <int VEC>
__device__ inline void batchnorm_load(const float* __restrict__ row, int t, int T, float v[kBnLaneFrames]) {
  if constexpr (VEC == 4) {
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < T) q = *reinterpret_cast<const float4*>(row + t);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < kBnLaneFrames; ++j) v[j] = t + j < T ? row[t + j] : 0.f;
  }
}

template <int VEC>
__device__ inline void batchnorm_store(float* __restrict__ row, int t, int T, const float v[kBnLaneFrames]) {
  if constexpr (VEC == 4) {
    if (t < T) *reinterpret_cast<float4*>(row + t) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < kBnLaneFrames; ++j)
      if (t + j < T) row[t + j] = v[j];
  }
}

// the shift of a channel's sums: its first element, or 0 when that is not finite (Inf - Inf would turn an Inf mean into a NaN)
__device__ inline float batchnorm_shift(const float* __restrict__ x, int c, int T) {
  const float s = x[int64_t(c) * T];
  return isfinite(s) ? s : 0.f;
}

__device__ inline double batchnorm_row_sum(double v) {
#pragma unroll
  for (int d = kBnRowLanes / 2; d >= 1; d /= 2) v += __shfl_xor(v, d, kBnRowLanes);
  return v;
}

// the ReLU's backward
template <bool RELU>
__device__ inline float batchnorm_gate(float g, float y) {
  return RELU && y <= 0.f ? 0.f : g;
}

template <int VEC>
__global__ __launch_bounds__(kBnThreads) void batchnorm_stats_kernel(const float* __restrict__ x, double* __restrict__ partial,
                                                                     const int64_t* __restrict__ tracked /* NULL: none */,
                                                                     int64_t* __restrict__ tracked_before, BatchNormArgs a) {
  const BatchNormLane p = batchnorm_lane(a);
  if (blockIdx.x == 0 && threadIdx.x == 0 && tracked) *tracked_before = *tracked;
  double s1 = 0.0, s2 = 0.0;
  if (p.valid) {
    const double shift = double(batchnorm_shift(x, p.c, a.T));
    float v[kBnLaneFrames];
    batchnorm_load<VEC>(x + p.row * a.T, p.t, a.T, v);
#pragma unroll
    for (int j = 0; j < kBnLaneFrames; ++j) {
      const double d = double(v[j]) - shift;
      const bool has = p.t + j < a.T;                              // frames past the row's end do not exist
      s1 = has ? s1 + d : s1;
      s2 = has ? fma(d, d, s2) : s2;
    }
  }
  s1 = batchnorm_row_sum(s1);
  s2 = batchnorm_row_sum(s2);
  if (p.l == 0 && p.valid) {
    double* dst = partial + ((p.b * a.tiles_t + p.tile) * a.C + p.c) * 2;
    dst[0] = s1;
    dst[1] = s2;
  }
}

// the two sums of channel blockIdx.x * kBnFoldChans + (threadIdx.x % kBnFoldChans) over its n partials, in the plan's order;
// true in the one lane a channel that holds them
__device__ inline bool batchnorm_fold(const double* __restrict__ partial, int64_t n, int C, double& s1, double& s2) {
  __shared__ double segs[kBnFoldSegs][kBnFoldChans][2];
  const int col = threadIdx.x % kBnFoldChans, q = threadIdx.x / kBnFoldChans;
  const int64_t c = int64_t(blockIdx.x) * kBnFoldChans + col;
  const int64_t len = batchnorm_fold_seg_len(n);
  const int64_t first = q * len, last = first + len < n ? first + len : n;
  double a1 = 0.0, a2 = 0.0;
  if (c < C) {
#pragma unroll 4                                                  // (loads in flight; the additions keep their order)
    for (int64_t t = first; t < last; ++t) {
      a1 += partial[(t * C + c) * 2];
      a2 += partial[(t * C + c) * 2 + 1];
    }
  }
  segs[q][col][0] = a1;
  segs[q][col][1] = a2;
  __syncthreads();
  if (q != 0 || c >= C) return false;
  const int nseg = int((n + len - 1) / len);                      // segments that hold a partial
  s1 = segs[0][col][0];
  s2 = segs[0][col][1];
  for (int i = 1; i < nseg; ++i) {
    s1 += segs[i][col][0];
    s2 += segs[i][col][1];
  }
  return true;
}

// grid: blocks of kBnFoldChans channels
__global__ __launch_bounds__(kBnThreads) void batchnorm_stats_fold_kernel(
    const double* __restrict__ partial, int64_t n, const float* __restrict__ x, int C, int T, double N, double eps,
    double momentum /* < 0: cumulative */, float* __restrict__ running_mean /* NULL: none */, float* __restrict__ running_var,
    int64_t* __restrict__ tracked /* NULL: none */, const int64_t* __restrict__ tracked_before, float* __restrict__ save_mean,
    float* __restrict__ save_invstd) {
  double s1, s2;
  const bool mine = batchnorm_fold(partial, n, C, s1, s2);
  const int64_t count = tracked ? *tracked_before + 1 : 0;
  if (tracked && blockIdx.x == 0 && threadIdx.x == 0) *tracked = count;
  if (!mine) return;
  const int c = blockIdx.x * kBnFoldChans + threadIdx.x;
  const double m1 = s1 / N;
  const double mean = double(batchnorm_shift(x, c, T)) + m1;
  double var = (s2 - s1 * m1) / N;
  var = var < 0.0 ? 0.0 : var;                                    // (a NaN is not below zero)
  save_mean[c] = float(mean);
  save_invstd[c] = float(1.0 / sqrt(var + eps));
  if (running_mean) {
    const double f = momentum < 0.0 ? 1.0 / double(count) : momentum;
    running_mean[c] = float((1.0 - f) * double(running_mean[c]) + f * mean);
    running_var[c] = float((1.0 - f) * double(running_var[c]) + f * (var * (N / (N - 1.0))));
  }
}

template <int VEC, bool RELU, bool RES, bool EVAL>
__global__ __launch_bounds__(kBnThreads) void batchnorm_apply_kernel(const float* __restrict__ x, const float* __restrict__ residual,
                                                                     float* __restrict__ y, const float* __restrict__ weight /* NULL: 1 */,
                                                                     const float* __restrict__ bias /* NULL: 0 */,
                                                                     const float* __restrict__ running_mean,
                                                                     const float* __restrict__ running_var, double eps,
                                                                     float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                                     BatchNormArgs a) {
  const BatchNormLane p = batchnorm_lane(a);
  if (!p.valid) return;
  float mean, invstd;
  if constexpr (EVAL) {
    mean = running_mean[p.c];
    invstd = float(1.0 / sqrt(double(running_var[p.c]) + eps));
    if (p.b == 0 && p.tile == 0 && p.l == 0) {
      save_mean[p.c] = mean;
      save_invstd[p.c] = invstd;
    }
  } else {
    mean = save_mean[p.c];
    invstd = save_invstd[p.c];
  }
  const float k = weight ? weight[p.c] * invstd : invstd;
  const float b0 = bias ? bias[p.c] : 0.f;
  float v[kBnLaneFrames], r[kBnLaneFrames];
  batchnorm_load<VEC>(x + p.row * a.T, p.t, a.T, v);
  if constexpr (RES) batchnorm_load<VEC>(residual + p.row * a.T, p.t, a.T, r);
#pragma unroll
  for (int j = 0; j < kBnLaneFrames; ++j) {
    float z = fmaf(v[j] - mean, k, b0);
    if constexpr (RES) z = z + r[j];
    if constexpr (RELU) z = z < 0.f ? 0.f : z;
    v[j] = z;
  }
  batchnorm_store<VEC>(y + p.row * a.T, p.t, a.T, v);
}

template <int VEC, bool RELU>
__global__ __launch_bounds__(kBnThreads) void batchnorm_grad_sums_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                         const float* __restrict__ g, const float* __restrict__ save_mean,
                                                                         double* __restrict__ partial, BatchNormArgs a) {
  const BatchNormLane p = batchnorm_lane(a);
  double s1 = 0.0, s2 = 0.0;
  if (p.valid) {
    const double mean = double(save_mean[p.c]);
    float xv[kBnLaneFrames], gv[kBnLaneFrames], yv[kBnLaneFrames];
    batchnorm_load<VEC>(x + p.row * a.T, p.t, a.T, xv);
    batchnorm_load<VEC>(g + p.row * a.T, p.t, a.T, gv);
    if constexpr (RELU) batchnorm_load<VEC>(y + p.row * a.T, p.t, a.T, yv);
#pragma unroll
    for (int j = 0; j < kBnLaneFrames; ++j) {
      const double gg = double(batchnorm_gate<RELU>(gv[j], RELU ? yv[j] : 0.f));
      const bool has = p.t + j < a.T;
      s1 = has ? s1 + gg : s1;
      s2 = has ? fma(gg, double(xv[j]) - mean, s2) : s2;
    }
  }
  s1 = batchnorm_row_sum(s1);
  s2 = batchnorm_row_sum(s2);
  if (p.l == 0 && p.valid) {
    double* dst = partial + ((p.b * a.tiles_t + p.tile) * a.C + p.c) * 2;
    dst[0] = s1;
    dst[1] = s2;
  }
}

// grid: blocks of kBnFoldChans channels
__global__ __launch_bounds__(kBnThreads) void batchnorm_grad_fold_kernel(const double* __restrict__ partial, int64_t n, int C, double N,
                                                                         const float* __restrict__ save_invstd,
                                                                         float* __restrict__ dw /* NULL: not wanted */,
                                                                         float* __restrict__ db /* NULL: not wanted */,
                                                                         float* __restrict__ coef /* NULL: not wanted */) {
  double s1, s2;
  if (!batchnorm_fold(partial, n, C, s1, s2)) return;
  const int c = blockIdx.x * kBnFoldChans + threadIdx.x;
  const double invstd = double(save_invstd[c]);
  if (db) db[c] = float(s1);
  if (dw) dw[c] = float(invstd * s2);
  if (coef) {
    coef[2 * c] = float(s1 / N);
    coef[2 * c + 1] = float(invstd * invstd * s2 / N);
  }
}

template <int VEC, bool RELU, bool BATCH>
__global__ __launch_bounds__(kBnThreads) void batchnorm_grad_x_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                      const float* __restrict__ g, const float* __restrict__ weight,
                                                                      const float* __restrict__ save_mean,
                                                                      const float* __restrict__ save_invstd, const float* __restrict__ coef,
                                                                      float* __restrict__ dx /* NULL: not wanted */,
                                                                      float* __restrict__ dres /* NULL: not wanted */, BatchNormArgs a) {
  const BatchNormLane p = batchnorm_lane(a);
  if (!p.valid) return;
  float gv[kBnLaneFrames], yv[kBnLaneFrames];
  batchnorm_load<VEC>(g + p.row * a.T, p.t, a.T, gv);
  if constexpr (RELU) {
    batchnorm_load<VEC>(y + p.row * a.T, p.t, a.T, yv);
#pragma unroll
    for (int j = 0; j < kBnLaneFrames; ++j) gv[j] = batchnorm_gate<true>(gv[j], yv[j]);
  }
  if (dres) batchnorm_store<VEC>(dres + p.row * a.T, p.t, a.T, gv);
  if (!dx) return;
  const float invstd = save_invstd[p.c];
  const float k = weight ? weight[p.c] * invstd : invstd;
  if constexpr (BATCH) {
    const float mean = save_mean[p.c], k1 = coef[2 * p.c], k2 = coef[2 * p.c + 1];
    float xv[kBnLaneFrames];
    batchnorm_load<VEC>(x + p.row * a.T, p.t, a.T, xv);
#pragma unroll
    for (int j = 0; j < kBnLaneFrames; ++j) gv[j] = fmaf(-(xv[j] - mean), k2, gv[j] - k1) * k;
  } else {
#pragma unroll
    for (int j = 0; j < kBnLaneFrames; ++j) gv[j] = gv[j] * k;
  }
  batchnorm_store<VEC>(dx + p.row * a.T, p.t, a.T, gv);
}

}  // namespace wekws
