// The Linear layers' weight and bias gradients for gfx950: grad_w (O, I) = g^T x and grad_bias (O) = the column sums of g, for
// x (R, I) and g (R, O) with O and I a few hundred and R = B T tens of thousands -- a split-K product whose arithmetic is stated
// in linear_wgrad_plan.h (chains of kWgradChain rows in float32 on the matrix cores, slices and fold in double) and whose bits
// are a function of the inputs and the shape.  Two launches, no floating-point atomics, no waits between workgroups.
//
//   linear_wgrad_partial<VEC>   workgroup (tile, slice): 4 waves own a 64 (O) x 64 (I) tile of grad_w over the slice's chains.
//                               Wave w owns the quadrant O [32 (w >> 1), +32) x I [32 (w & 1), +32) as 2 x 2 tiles of
//                               v_mfma_f32_16x16x4_f32: four independent accumulators.  A stage is 32 rows of g and of x in LDS
//                               as [row][64 columns] with a row stride of 80 floats; lane l reads A = g[k = l >> 4][o = l & 15]
//                               and B = x[k = l >> 4][i = l & 15], so a lane's result register j is
//                               grad_w[o = 4 (l >> 4) + j][i = l & 15] of its 16 x 16 tile.  Two LDS buffers: stage s + 1 is
//                               fetched into registers before stage s is computed and stored to the other buffer after it, one
//                               barrier a stage.  VEC: 16-byte global loads (O % 4 == 0, I % 4 == 0, 16-byte aligned bases);
//                               otherwise four scalar loads with the same bits.  At every chain boundary the 16 accumulators
//                               are added into 16 doubles and zeroed.  Rows past the slice's end and columns past O / I are
//                               zeros in LDS; padded results are never stored.  The workgroups of I-tile 0 also sum the columns
//                               of the g stage they hold (wave 0, one column a lane).  Without grad_w only those run, and no MFMA.
//                               BCT: the operands are laid out (B, C, T) -- the activations of a pointwise Conv1d
//                               (pointwise_conv_plan.h) -- so row r = b T + t of column c is at base + ((r / T) C + c) T + r % T
//                               and the contiguous axis is k.  A thread then fetches rows 4 (tid >> 6) + 16 j + 0 .. 3 of column
//                               tid & 63 -- one 16-byte load where T % 4 == 0 and the bases are 16-byte aligned, four scalar loads
//                               that step over the batch-row boundary otherwise -- and stores them to the same LDS layout by four
//                               4-byte stores, a wave's 64 lanes on 64 consecutive banks: no conflict.  A stage may straddle
//                               batch rows.  Everything after the fetch is the row-major kernel's, so are the bits.
//   linear_wgrad_fold           one lane per element of grad_w and of grad_bias: the slices' doubles added in ascending order,
//                               eight loads in flight, rounded once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "linear_wgrad_plan.h"

namespace wekws {

typedef float wgrad_f32x4 __attribute__((ext_vector_type(4)));

template <bool VEC>
__device__ inline float4 wgrad_fetch(const float* __restrict__ base, int64_t row, int64_t row_end, int64_t ld, int col, int cols) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row >= row_end) return v;
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

// (B, C, T) operands: rows row .. row + 3 of column col, row = b T + t.  VEC: T % 4 == 0 and row % 4 == 0, so the four rows lie
// in one batch row, 16-byte aligned, and are inside row_end together (R % 4 == 0 and the chains' ends are multiples of 4).
template <bool VEC>
__device__ inline float4 wgrad_fetch_bct(const float* __restrict__ base, int64_t row, int64_t row_end, int64_t b, int64_t t, int64_t T,
                                         int col, int cols) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (col >= cols || row >= row_end) return v;
  if (VEC) {
    v = *reinterpret_cast<const float4*>(base + (b * cols + col) * T + t);
  } else {
    float e[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (row + u < row_end) e[u] = base[(b * cols + col) * T + t];
      if (++t == T) {
        t = 0;
        ++b;
      }
    }
    v = make_float4(e[0], e[1], e[2], e[3]);
  }
  return v;
}

// The x operand of a tap of a dense Conv1d (dense_conv_plan.h): rows row .. row + 3 of column col, row = b T + t, are
// x[b][col][t + shift] of x (B, cols, Tx), zeros where t + shift is outside [0, Tx).  Scalar loads.
__device__ inline float4 wgrad_fetch_tap(const float* __restrict__ base, int64_t row, int64_t row_end, int64_t b, int64_t t, int64_t T,
                                         int64_t Tx, int64_t shift, int col, int cols) {
  float e[4] = {0.f, 0.f, 0.f, 0.f};
  if (col < cols && row < row_end) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t n = t + shift;
      if (row + u < row_end && n >= 0 && n < Tx) e[u] = base[(b * cols + col) * Tx + n];
      if (++t == T) {
        t = 0;
        ++b;
      }
    }
  }
  return make_float4(e[0], e[1], e[2], e[3]);
}

// T: frames of a batch row of the (B, C, T) operands (BCT); unused otherwise.  TAP (with BCT): blockIdx.y is a tap of a dense
// Conv1d -- g is (B, O, T), x is (B, I, Tx) read at the frame shift tap * dil - pad (wgrad_fetch_tap), the tap's partials go
// tap * tap_stride doubles further into ws_w, and tap 0 alone sums the bias.  Everything after the fetch is unchanged.
template <bool VEC, bool BCT = false, bool TAP = false>
__global__ __launch_bounds__(kWgradThreads) void linear_wgrad_partial(const float* __restrict__ x, const float* __restrict__ g,
                                                                      int64_t R, int O, int I, int tiles_i, int64_t chains_per_slice,
                                                                      int64_t o_pad, int64_t i_pad, double* __restrict__ ws_w,
                                                                      double* __restrict__ ws_b, int64_t T, int64_t Tx, int dil, int pad,
                                                                      int64_t tap_stride) {
  static_assert(BCT || !TAP, "the per-tap fetch is a (B, C, T) fetch");
  const int64_t shift = TAP ? int64_t(blockIdx.y) * dil - pad : 0;
  if (TAP) {
    if (ws_w) ws_w += blockIdx.y * tap_stride;
    if (blockIdx.y) ws_b = nullptr;
  }
  constexpr int S = kWgradStride, ST = kWgradStage, BUF = kWgradStage * kWgradStride;
  constexpr int kStagesPerChain = kWgradChain / kWgradStage;
  __shared__ __attribute__((aligned(16))) float lds[2 * 2 * BUF];      // [buffer][g, x][row][S]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const bool want_w = ws_w != nullptr;
  const int64_t tiles_o = o_pad / kWgradTile;
  const int64_t tiles = tiles_o * tiles_i;
  const int64_t slice = blockIdx.x / tiles;
  const int tile = int(blockIdx.x - slice * tiles);
  const int to = tile / tiles_i, ti = tile - to * tiles_i;
  const int o_base = to * kWgradTile, i_base = ti * kWgradTile;
  const bool want_b = ws_b != nullptr && ti == 0;

  const int64_t r_begin = slice * chains_per_slice * kWgradChain;
  const int64_t r_stop = r_begin + chains_per_slice * kWgradChain;
  const int64_t r_end = r_stop < R ? r_stop : R;
  const int stages = int((r_end - r_begin + ST - 1) / ST);

  // what this thread fetches of a stage: rows frow and frow + 16, columns fcol .. fcol + 3 of the tile; BCT: rows
  // frow + 16 j + 0 .. 3 of column fcol, with (fb[j], ft[j]) the batch row and frame of the first of them
  const int frow = BCT ? (tid >> 6) * 4 : tid >> 4, fcol = BCT ? (tid & 63) : (tid & 15) * 4;
  float4 gq[2], xq[2];
  int64_t fb[2] = {0, 0}, ft[2] = {0, 0};
  if (BCT) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t r0 = r_begin + frow + 16 * j;
      fb[j] = r0 / T;
      ft[j] = r0 - fb[j] * T;
    }
  }
  auto fetch = [&](int s) {                                  // BCT: called for s = 0, 1, 2, ... in order
    const int64_t r0 = r_begin + int64_t(s) * ST + frow;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (BCT) {
        gq[j] = wgrad_fetch_bct<VEC>(g, r0 + 16 * j, r_end, fb[j], ft[j], T, o_base + fcol, O);
        xq[j] = !want_w ? make_float4(0.f, 0.f, 0.f, 0.f)
                : TAP   ? wgrad_fetch_tap(x, r0 + 16 * j, r_end, fb[j], ft[j], T, Tx, shift, i_base + fcol, I)
                        : wgrad_fetch_bct<VEC>(x, r0 + 16 * j, r_end, fb[j], ft[j], T, i_base + fcol, I);
        ft[j] += ST;                                         // the same rows of the next stage
        while (ft[j] >= T) {
          ft[j] -= T;
          ++fb[j];
        }
      } else {
        gq[j] = wgrad_fetch<VEC>(g, r0 + 16 * j, r_end, O, o_base + fcol, O);
        xq[j] = want_w ? wgrad_fetch<VEC>(x, r0 + 16 * j, r_end, I, i_base + fcol, I) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  auto stash = [&](int s) {
    float* const bg = lds + (s & 1) * 2 * BUF;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (BCT) {                                             // the transposing store: a wave's lanes on 64 consecutive banks
        float* const pg = bg + (frow + 16 * j) * S + fcol;
        pg[0] = gq[j].x, pg[S] = gq[j].y, pg[2 * S] = gq[j].z, pg[3 * S] = gq[j].w;
        if (want_w) pg[BUF] = xq[j].x, pg[BUF + S] = xq[j].y, pg[BUF + 2 * S] = xq[j].z, pg[BUF + 3 * S] = xq[j].w;
      } else {
        *reinterpret_cast<float4*>(bg + (frow + 16 * j) * S + fcol) = gq[j];
        if (want_w) *reinterpret_cast<float4*>(bg + BUF + (frow + 16 * j) * S + fcol) = xq[j];
      }
    }
  };

  wgrad_f32x4 acc[2][2];
  double dacc[2][2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      acc[m][n] = wgrad_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) dacc[m][n][j] = 0.0;
    }
  float bacc = 0.f;
  double bsum = 0.0;
  const int wo = (wave >> 1) * 32, wi = (wave & 1) * 32;

  fetch(0);
  stash(0);
  __syncthreads();
  for (int s = 0; s < stages; ++s) {
    if (s + 1 < stages) fetch(s + 1);
    const float* const bg = lds + (s & 1) * 2 * BUF;
    const float* const bx = bg + BUF;
    if (want_w) {
      const float* const ap = bg + lq * S + wo + l15;
      const float* const bp = bx + lq * S + wi + l15;
#pragma unroll
      for (int kk = 0; kk < ST / 4; ++kk) {
        const float a0 = ap[kk * 4 * S], a1 = ap[kk * 4 * S + 16];
        const float b0 = bp[kk * 4 * S], b1 = bp[kk * 4 * S + 16];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    if (want_b && wave == 0) {
#pragma unroll
      for (int r = 0; r < ST; ++r) bacc += bg[r * S + lane];
    }
    if ((s + 1) % kStagesPerChain == 0 || s + 1 == stages) {           // the chain ends here
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
#pragma unroll
          for (int j = 0; j < 4; ++j) dacc[m][n][j] += double(acc[m][n][j]);
          acc[m][n] = wgrad_f32x4{0.f, 0.f, 0.f, 0.f};
        }
      bsum += double(bacc);
      bacc = 0.f;
    }
    if (s + 1 < stages) stash(s + 1);
    __syncthreads();
  }

  if (want_w) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int o = o_base + wo + 16 * m + 4 * lq + j, i = i_base + wi + 16 * n + l15;
          if (o < O && i < I) ws_w[(slice * o_pad + o) * i_pad + i] = dacc[m][n][j];
        }
  }
  if (want_b && wave == 0 && o_base + lane < O) ws_b[slice * o_pad + o_base + lane] = bsum;
}

// element e of [first, first + count): e < O I is grad_w[e], the rest grad_bias[e - O I].  blockIdx.y is a tap of a dense Conv1d
// (one tap, stride 0, everywhere else): its partials lie tap * tap_stride doubles further, its element e of grad_w is
// grad_w[e * taps + tap] -- (O, I, taps), taps contiguous -- and tap 0 alone folds the bias.
__global__ __launch_bounds__(kWgradFoldThreads) void linear_wgrad_fold(const double* __restrict__ ws, int O, int I, int64_t slices,
                                                                       int64_t o_pad, int64_t i_pad, int64_t bias_offset,
                                                                       int64_t first, int64_t last, float* __restrict__ grad_w,
                                                                       float* __restrict__ grad_bias, int64_t tap_stride) {
  const int64_t e = first + int64_t(blockIdx.x) * kWgradFoldThreads + threadIdx.x;
  if (e >= last) return;
  const int64_t n_w = int64_t(O) * I;
  const int64_t tap = blockIdx.y, taps = gridDim.y;
  if (e >= n_w && tap) return;
  ws += tap * tap_stride;
  const double* p;
  int64_t stride;
  float* out;
  if (e < n_w) {
    const int64_t o = e / I, i = e - o * I;
    p = ws + o * i_pad + i;
    stride = o_pad * i_pad;
    out = grad_w + e * taps + tap;
  } else {
    p = ws + bias_offset + (e - n_w);
    stride = o_pad;
    out = grad_bias + (e - n_w);
  }
  double sum = 0.0;
  int64_t k = 0;
  for (; k + 8 <= slices; k += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(k + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += v[u];
  }
  for (; k < slices; ++k) sum += p[k * stride];
  *out = float(sum);
}

}  // namespace wekws
