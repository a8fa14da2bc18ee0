// The pointwise (kernel_size 1) Conv1d of the TCN and MDTC blocks for gfx950: y[b][m][t] = (bias[m] +) sum_k W(m, k) x[b][k][t]
// for x (B, K, T) and y (B, M, T), the forward product (W(m, k) = w[m][k], K = Ci, M = Co) and the input gradient
// (W(m, k) = w[k][m], K = Co, M = Ci, x the output gradient) of pointwise_conv_plan.h.  The weight and bias gradients are
// linear_wgrad.hip.h's kernels with the (B, C, T) fetch.
//
//   pointwise_conv_mm<TRANS, BIAS, VECX, VECW>
//       workgroup (batch row, frame tile, channel tile): 4 waves own a 64 (channels m) x 64 (frames t) tile of y[b].  Wave v
//       owns the quadrant m [32 (v >> 1), +32) x t [32 (v & 1), +32) as 2 x 2 tiles of v_mfma_f32_16x16x4_f32: four
//       independent accumulators, each the fmaf chain over k ascending from +0.  A stage is 32 k rows of the weight and of x in
//       LDS as [k][64 columns] with a row stride of 80 floats -- linear_wgrad.hip.h's stage: lane l reads A = W[k = l >> 4]
//       [m = l & 15] and B = x[k = l >> 4][t = l & 15], so a lane's result register j is y[m = 4 (l >> 4) + j][t = l & 15] of
//       its 16 x 16 tile.  Two LDS buffers, stage s + 1 fetched into registers before stage s is computed and stored after it,
//       one barrier a stage.
//       x: row k of the stage is x[b][k][t0 .. t0 + 64), contiguous; a thread fetches rows tid >> 4 and + 16, frames
//       4 (tid & 15) + 0 .. 3.  VECX: 16-byte loads (T % 4 == 0, 16-byte aligned base); otherwise four scalar loads.
//       weight, TRANS (the input gradient): the stage's rows are rows of w, fetched like x (VECW: Ci % 4 == 0, aligned base).
//       weight, not TRANS (the forward): the stage is the transposed tile of w, whose contiguous axis is k.  A thread fetches
//       k = 4 (tid >> 6) + 16 j + 0 .. 3 of row m = tid & 63 (VECW: one 16-byte load) and stores them by four 4-byte stores, a
//       wave's 64 lanes on 64 consecutive banks: no conflict.
//       Frames past T and channels past K / M are zeros in LDS and are never stored.  BIAS: one float32 addition at the store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pointwise_conv_plan.h"

namespace wekws {

typedef float pw_f32x4 __attribute__((ext_vector_type(4)));

// columns col .. col + 3 of row `row` of a row-major operand with `cols` columns and `rows` rows; zeros outside
template <bool VEC>
__device__ inline float4 pw_fetch_row(const float* __restrict__ base, int row, int rows, int64_t ld, int64_t col, int64_t cols) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row >= rows) return v;
  const float* const p = base + row * ld + col;
  if (VEC) {
    if (col < cols) v = *reinterpret_cast<const float4*>(p);        // cols % 4 == 0: the four are inside together
  } else {
    if (col < cols) v.x = p[0];
    if (col + 1 < cols) v.y = p[1];
    if (col + 2 < cols) v.z = p[2];
    if (col + 3 < cols) v.w = p[3];
  }
  return v;
}

// rows k .. k + 3 of column m of the transposed weight: w[m][k .. k + 3], contiguous; zeros outside
template <bool VEC>
__device__ inline float4 pw_fetch_col(const float* __restrict__ w, int m, int M, int64_t ld, int k, int K) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (m >= M) return v;
  const float* const p = w + m * ld + k;
  if (VEC) {
    if (k < K) v = *reinterpret_cast<const float4*>(p);             // K % 4 == 0: the four are inside together
  } else {
    if (k < K) v.x = p[0];
    if (k + 1 < K) v.y = p[1];
    if (k + 2 < K) v.z = p[2];
    if (k + 3 < K) v.w = p[3];
  }
  return v;
}

// One stage of a wave's quadrant (dense_conv.hip.h uses it too): ap and bp are the lane's first elements of the weight and the x
// stage, [k][kPwStride]; the four accumulators take the stage's 32 k in ascending order.
__device__ inline void pw_stage_product(const float* __restrict__ ap, const float* __restrict__ bp, pw_f32x4 (&acc)[2][2]) {
  constexpr int S = kPwStride;
#pragma unroll
  for (int kk = 0; kk < kPwStage / 4; ++kk) {
    const float a0 = ap[kk * 4 * S], a1 = ap[kk * 4 * S + 16];
    const float b0 = bp[kk * 4 * S], b1 = bp[kk * 4 * S + 16];
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
  }
}

// A wave's quadrant to yb (M, T): the lane's rows o0 + 16 m + j and columns t0 + 16 n; BIAS: one float32 addition at the store.
template <bool BIAS>
__device__ inline void pw_store_quadrant(const pw_f32x4 (&acc)[2][2], float* __restrict__ yb, const float* __restrict__ bias, int o0, int M,
                                         int64_t t0, int64_t T) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = o0 + 16 * m + j;
      if (o >= M) continue;
      const float add = BIAS ? bias[o] : 0.f;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int64_t t = t0 + 16 * n;
        if (t < T) yb[int64_t(o) * T + t] = BIAS ? acc[m][n][j] + add : acc[m][n][j];
      }
    }
}

// ldw: the row length of w, Ci
template <bool TRANS, bool BIAS, bool VECX, bool VECW>
__global__ __launch_bounds__(kPwThreads) void pointwise_conv_mm(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float* __restrict__ y, int K, int M,
                                                                int T, int tiles_m, int tiles_t, int ldw) {
  constexpr int S = kPwStride, ST = kPwStage, BUF = kPwStage * kPwStride;
  __shared__ __attribute__((aligned(16))) float lds[2 * 2 * BUF];      // [buffer][weight, x][k][S]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int tm = int(blockIdx.x % unsigned(tiles_m));
  const unsigned bt = blockIdx.x / unsigned(tiles_m);
  const int tt = int(bt % unsigned(tiles_t));
  const int64_t b = bt / unsigned(tiles_t);
  const int m_base = tm * kPwTile;
  const int64_t t_base = int64_t(tt) * kPwTile;
  const float* const xb = x + b * K * T;
  float* const yb = y + b * M * T;
  const int stages = (K + ST - 1) / ST;

  // what this thread fetches of a stage: rows frow and frow + 16, columns fcol .. fcol + 3 of the tile; of the forward's
  // weight, k = crow + 16 j + 0 .. 3 of column lane
  const int frow = tid >> 4, fcol = (tid & 15) * 4;
  const int crow = wave * 4;
  float4 wq[2], xq[2];
  auto fetch = [&](int s) {
    const int k0 = s * ST;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      xq[j] = pw_fetch_row<VECX>(xb, k0 + frow + 16 * j, K, T, t_base + fcol, T);
      wq[j] = TRANS ? pw_fetch_row<VECW>(w, k0 + frow + 16 * j, K, ldw, m_base + fcol, M)
                    : pw_fetch_col<VECW>(w, m_base + lane, M, ldw, k0 + crow + 16 * j, K);
    }
  };
  auto stash = [&](int s) {
    float* const bw = lds + (s & 1) * 2 * BUF;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *reinterpret_cast<float4*>(bw + BUF + (frow + 16 * j) * S + fcol) = xq[j];
      if (TRANS) {
        *reinterpret_cast<float4*>(bw + (frow + 16 * j) * S + fcol) = wq[j];
      } else {                                                         // the transposing store
        float* const p = bw + (crow + 16 * j) * S + lane;
        p[0] = wq[j].x, p[S] = wq[j].y, p[2 * S] = wq[j].z, p[3 * S] = wq[j].w;
      }
    }
  };

  pw_f32x4 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = pw_f32x4{0.f, 0.f, 0.f, 0.f};
  const int wm = (wave >> 1) * 32, wt = (wave & 1) * 32;

  fetch(0);
  stash(0);
  __syncthreads();
  for (int s = 0; s < stages; ++s) {
    if (s + 1 < stages) fetch(s + 1);
    const float* const bw = lds + (s & 1) * 2 * BUF;
    pw_stage_product(bw + lq * S + wm + l15, bw + BUF + lq * S + wt + l15, acc);
    if (s + 1 < stages) stash(s + 1);
    __syncthreads();
  }

  pw_store_quadrant<BIAS>(acc, yb, bias, m_base + wm + 4 * lq, M, t_base + wt + l15, T);
}

}  // namespace wekws
