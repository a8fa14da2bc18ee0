// The dense (groups 1) dilated Conv1d of the TCN's CnnBlock for gfx950: the forward product and the input gradient of
// dense_conv_plan.h as one kernel, a sum over taps of pointwise_conv.hip.h's product:
//     y[b][m][n] = (bias[m] +) sum_k sum_c W_k(m, c) v[b][c][n + shift_k]        v an arithmetic zero outside [0, Tv)
// for v (B, C, Tv) and y (B, M, N).  Forward: v = x, C = Ci, M = Co, N = Tout, W_k(m, c) = w[m][c][k], shift_k = k d - left_pad.
// Input gradient (TRANS): v = the output gradient, C = Co, M = Ci, N = Tin, W_k(m, c) = w[c][m][k], shift_k = left_pad - k d.
// The weight and bias gradients are linear_wgrad.hip.h's kernels with the per-tap (B, C, T) fetch.
//
//   dense_conv_mm<TRANS, BIAS, VECX>
//       pointwise_conv_mm's workgroup, tile, stage and MFMA order (pw_stage_product), its LDS layout and its store
//       (pw_store_quadrant); the stage loop runs over taps and, inside a tap, over stages of 32 channels, so an accumulator is the
//       fmaf chain over j = k C + c ascending from +0.
//       v: row c of a tap's stage is v[b][c][n0 + shift_k .. + 64): the tile's frames shifted.  A thread fetches rows tid >> 4 and
//       + 16, columns 4 (tid & 15) + 0 .. 3.  VECX (Tv % 4 == 0, 16-byte aligned base): one 16-byte load where the tap's shift is
//       a multiple of 4 and the four frames are inside [0, Tv); four scalar loads, each a zero outside [0, Tv), otherwise.  The
//       choice is uniform over a stage but for the tiles on the rows' edges.  A tap's frames are fetched again for the next tap;
//       they come from the cache (DESIGN.md 3.27 has why the stage with a halo was not taken).
//       weight: its contiguous axis is k, so a stage's operand has stride K in both forms and is fetched by scalar loads at that
//       stride (the weight is a few hundred KB and stays in the cache); stored to LDS as pointwise_conv_mm stores its weight.
//       Frames past N and channels past C / M are zeros in LDS and are never stored.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dense_conv_plan.h"
#include "pointwise_conv.hip.h"

namespace wekws {

// frames n .. n + 3 (n may be negative) of row `row` of vb (rows, Tv); zeros for a row past `rows` and for frames outside [0, Tv)
template <bool VEC>
__device__ inline float4 dense_fetch_frames(const float* __restrict__ vb, int row, int rows, int64_t Tv, int64_t n) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row >= rows || n >= Tv || n + 3 < 0) return v;
  const float* const p = vb + row * Tv + n;
  if (VEC && (n & 3) == 0 && n >= 0 && n + 4 <= Tv) return *reinterpret_cast<const float4*>(p);
  if (n >= 0) v.x = p[0];
  if (n + 1 >= 0 && n + 1 < Tv) v.y = p[1];
  if (n + 2 >= 0 && n + 2 < Tv) v.z = p[2];
  if (n + 3 < Tv) v.w = p[3];
  return v;
}

// four weights at stride `step` from w[row * ld + col * step]: elements (row, col .. col + 3) of a (rows, cols) operand whose
// columns are `step` apart; zeros outside
__device__ inline float4 dense_fetch_weights(const float* __restrict__ w, int row, int rows, int64_t ld, int col, int cols, int64_t step) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row >= rows) return v;
  const float* const p = w + row * ld + col * step;
  if (col < cols) v.x = p[0];
  if (col + 1 < cols) v.y = p[step];
  if (col + 2 < cols) v.z = p[2 * step];
  if (col + 3 < cols) v.w = p[3 * step];
  return v;
}

// C reduction channels, M output channels, Tv frames of v, N frames of y; shift_k = shift0 + k shift_step; Ci: the weight's middle
// extent (w is (Co, Ci, taps))
template <bool TRANS, bool BIAS, bool VECX>
__global__ __launch_bounds__(kPwThreads) void dense_conv_mm(const float* __restrict__ v, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ y, int C, int M, int Tv,
                                                            int N, int taps, int shift0, int shift_step, int Ci, int tiles_m,
                                                            int tiles_n) {
  constexpr int S = kPwStride, ST = kPwStage, BUF = kPwStage * kPwStride;
  __shared__ __attribute__((aligned(16))) float lds[2 * 2 * BUF];      // [buffer][weight, v][c][S]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int tm = int(blockIdx.x % unsigned(tiles_m));
  const unsigned bt = blockIdx.x / unsigned(tiles_m);
  const int tn = int(bt % unsigned(tiles_n));
  const int64_t b = bt / unsigned(tiles_n);
  const int m_base = tm * kPwTile;
  const int64_t n_base = int64_t(tn) * kPwTile;
  const float* const vb = v + b * C * Tv;
  float* const yb = y + b * M * N;
  const int cstages = (C + ST - 1) / ST;
  const int stages = taps * cstages;

  // what this thread fetches of a stage: rows frow and frow + 16, columns fcol .. fcol + 3 of the tile; of the forward's weight,
  // c = crow + 16 j + 0 .. 3 of column lane
  const int frow = tid >> 4, fcol = (tid & 15) * 4;
  const int crow = wave * 4;
  const int64_t ldw = int64_t(Ci) * taps;                                // between two rows of w
  float4 wq[2], xq[2];
  auto fetch = [&](int s) {
    const int k = s / cstages, c0 = (s - k * cstages) * ST;
    const int64_t n0 = n_base + fcol + shift0 + k * shift_step;
    const float* const wk = w + k;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      xq[j] = dense_fetch_frames<VECX>(vb, c0 + frow + 16 * j, C, Tv, n0);
      // TRANS: row c of the stage is w[c][m_base + fcol ..][k], columns taps apart; else column m = lane is w[m][c ..][k]
      wq[j] = TRANS ? dense_fetch_weights(wk, c0 + frow + 16 * j, C, ldw, m_base + fcol, M, taps)
                    : dense_fetch_weights(wk, m_base + lane, M, ldw, c0 + crow + 16 * j, C, taps);
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
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;

  fetch(0);
  stash(0);
  __syncthreads();
  for (int s = 0; s < stages; ++s) {
    if (s + 1 < stages) fetch(s + 1);
    const float* const bw = lds + (s & 1) * 2 * BUF;
    pw_stage_product(bw + lq * S + wm + l15, bw + BUF + lq * S + wn + l15, acc);
    if (s + 1 < stages) stash(s + 1);
    __syncthreads();
  }
  pw_store_quadrant<BIAS>(acc, yb, bias, m_base + wm + 4 * lq, M, n_base + wn + l15, N);
}

}  // namespace wekws
