// The trainable depthwise Conv1d on the device: nn.Conv1d(C, C, K, dilation=d, groups=C) behind an F.pad(x, (P, 0)) -- the
// reference's DsCnnBlock.cnn[0] (wekws/model/tcn.py:102-107) and DSDilatedConv1d.conv (wekws/model/mdtc.py:37-46) -- and its
// autograd, over a (B, C, T) float32 tensor.  depthwise_conv_plan.h has the tap table, the tiles and the workspace.  Time is
// the contiguous axis: a row is one (b, c) pair, 32 lanes run along t of one row and a tap is a shift along the lanes.  Three
// kernels:
//   depthwise_conv_fir_kernel<VEC, BWD>   one workgroup owns kDwConvFirTile output frames of kDwConvRows rows.  It copies those
//                        frames and their window into LDS once, the zeros in front of a row (and past its end) written as zeros,
//                        with the rows' coefficients and bias beside them; every lane adds its K products by exact float32 fmaf
//                        in the table's order into four frames 32 apart, and the tile leaves through LDS.  BWD = false: y from
//                        x, starting from the bias (or +0); the padding is arithmetic zeros (an Inf tap makes the first P frames
//                        NaN, as the reference's padding does).  BWD = true: dx from g, the same taps with the delays negated,
//                        terms outside [0, Tout) left out.  VEC = 4: 16-byte global accesses (both row lengths % 4 == 0,
//                        aligned bases); VEC = 1: scalars.  VEC only changes the copies: the products and their order are the same.
//   depthwise_conv_tap_grad_kernel<VEC>   one workgroup owns kDwConvGradTile frames of kDwConvRows rows; per tap and for the
//                        bias a lane adds g * x over its four frames in ascending order in double (the product of two floats is
//                        exact there), the 32 lanes of a row are combined by a fixed butterfly, and one partial per (batch row,
//                        tile, channel, tap or bias) goes to the workspace as (B * tiles, C, K + 1) doubles.
//   depthwise_conv_fold_kernel            adds the partials of kDwConvFoldCols (channel, tap) pairs: up to kDwConvFoldSegs segments
//                        of consecutive partials in ascending order, then the segments' sums in ascending order, rounds to
//                        float32 once and writes grad_w / grad_bias.
// A row's y and dx depend on that row alone; the order of the tap gradient's additions is a function of the shape alone.  No
// floating-point atomics; nothing synchronises, allocates or reads on the host.  This object is built with -fno-slp-vectorize
// (DESIGN.md 3.8): the fmaf chains and the double sums stay scalar instructions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "depthwise_conv_plan.h"

namespace wekws {

// what the kernels are told.  A kernel reads rows of `Lin` frames and owns tiles of rows of `Lout` frames; LDS column j of a
// tile that starts at frame t0 holds source frame t0 + delta + j (before the 16-byte alignment of the copy), and tap k reads
// column i + off[k] for output frame t0 + i.
struct DepthwiseConvArgs {
  int64_t rows;                               // B * C
  int C, K;
  int Lin, Lout;
  int delta;                                  // forward, tap gradient: -P;  input gradient: P - halo
  int halo;                                   // window - 1
  int tiles_t;                                // frame tiles of a row (of the kernel that is launched)
  int stride;                                 // floats of a staged row in LDS
  int16_t off[kDwConvMaxTaps];                // forward, tap gradient: halo - delay = k d;  input gradient: delay
};

// lds[r * stride + j] = src[row0 + r, a0 + j] for r < kDwConvRows, j < n (n % 4 == 0); 0 where the frame is outside [0, L) or
// the row is >= rows.  VEC == 4: a0 % 4 == 0 and L % 4 == 0, so four frames are inside or outside as a whole.
template <int VEC>
__device__ inline void depthwise_conv_stage(float* __restrict__ lds, int stride, const float* __restrict__ src, int64_t row0,
                                            int64_t rows, int L, int a0, int n) {
  const int cols = n / VEC;
  for (int i = threadIdx.x; i < kDwConvRows * cols; i += kDwConvThreads) {
    const int r = i / cols, j = (i % cols) * VEC;
    const int f = a0 + j;
    const int64_t row = row0 + r;
    const bool in = row < rows && f >= 0 && f < L;
    if constexpr (VEC == 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in) v = *reinterpret_cast<const float4*>(src + row * L + f);
      *reinterpret_cast<float4*>(lds + r * stride + j) = v;
    } else {
      lds[r * stride + j] = in ? src[row * L + f] : 0.f;
    }
  }
}

constexpr int kDwConvLaneFrames = kDwConvFirTile / kDwConvRowLanes;     // 4: frames a lane owns, kDwConvRowLanes apart
static_assert(kDwConvFirTile == kDwConvGradTile, "the FIR and the tap-gradient kernels share the lane mapping");
static_assert(kDwConvRowLanes == 32, "a row is half a wave: the butterfly below runs over 32 lanes");

template <int VEC, bool BWD>
__global__ __launch_bounds__(kDwConvThreads) void depthwise_conv_fir_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                            const float* __restrict__ w,
                                                                            const float* __restrict__ bias /* NULL: none */,
                                                                            DepthwiseConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float depthwise_conv_lds[];
  constexpr int kCoefs = kDwConvMaxTaps + 1;                      // a row's taps, then its bias
  float* xs = depthwise_conv_lds;                                 // [rows][stride]
  float* ys = xs + kDwConvRows * a.stride;                        // [rows][kDwConvFirTile]
  float* cs = ys + kDwConvRows * kDwConvFirTile;                  // [rows][kCoefs]
  const int t0 = int(blockIdx.x % a.tiles_t) * kDwConvFirTile;
  const int64_t row0 = int64_t(blockIdx.x / a.tiles_t) * kDwConvRows;
  const int base = t0 + a.delta;                                  // the source frame of output frame t0 under a tap of offset 0
  const int a0 = base & ~3;                                       // ... rounded down to a multiple of four (two's complement)
  const int s = base - a0;
  depthwise_conv_stage<VEC>(xs, a.stride, in, row0, a.rows, a.Lin, a0, (s + kDwConvFirTile + a.halo + 3) & ~3);
  for (int i = threadIdx.x; i < kDwConvRows * (a.K + 1); i += kDwConvThreads) {
    const int r = i / (a.K + 1), k = i % (a.K + 1);
    const int64_t row = row0 + r;
    float v = 0.f;
    if (row < a.rows) {
      const int c = int(row % a.C);
      if (k < a.K) v = w[int64_t(c) * a.K + k];
      else if (!BWD && bias) v = bias[c];
    }
    cs[r * kCoefs + (k < a.K ? k : kDwConvMaxTaps)] = v;
  }
  __syncthreads();
  const int r = threadIdx.x / kDwConvRowLanes, l = threadIdx.x % kDwConvRowLanes;
  const float* xr = xs + r * a.stride + l + s;
  float acc[kDwConvLaneFrames];
#pragma unroll
  for (int m = 0; m < kDwConvLaneFrames; ++m) acc[m] = BWD ? 0.f : cs[r * kCoefs + kDwConvMaxTaps];   // the bias, or +0
  for (int k = 0; k < a.K; ++k) {
    const int off = a.off[k];
    const float wk = cs[r * kCoefs + k];
#pragma unroll
    for (int m = 0; m < kDwConvLaneFrames; ++m) {
      const int i = l + m * kDwConvRowLanes;
      const float p = fmaf(wk, xr[m * kDwConvRowLanes + off], acc[m]);
      const int f = base + i + off;                               // the frame of g the term reads
      acc[m] = (!BWD || (f >= 0 && f < a.Lin)) ? p : acc[m];      // no such term: the sum stays as it is
    }
  }
#pragma unroll
  for (int m = 0; m < kDwConvLaneFrames; ++m) ys[r * kDwConvFirTile + l + m * kDwConvRowLanes] = acc[m];
  __syncthreads();
  constexpr int kCols = kDwConvFirTile / VEC;
  for (int i = threadIdx.x; i < kDwConvRows * kCols; i += kDwConvThreads) {
    const int rr = i / kCols, j = (i % kCols) * VEC;
    const int64_t row = row0 + rr;
    const int t = t0 + j;
    if (row >= a.rows || t >= a.Lout) continue;                   // VEC == 4: Lout % 4 == 0, four frames inside or outside
    float* o = out + row * a.Lout + t;
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(ys + rr * kDwConvFirTile + j);
    else *o = ys[rr * kDwConvFirTile + j];
  }
}

// partial[b * tiles_t + tile][c][k] = the sum over the tile's frames of g[t] * xp[t + k d - P] (k < K) or of g[t] (k == K), in
// double: per lane over its frames in ascending order, then the 32 lanes by the butterfly 16, 8, 4, 2, 1.  Columns
// [k_begin, k_end) are computed: a gradient nobody wants drops its work.
template <int VEC>
__global__ __launch_bounds__(kDwConvThreads) void depthwise_conv_tap_grad_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                                 double* __restrict__ partial, DepthwiseConvArgs a,
                                                                                 int k_begin, int k_end) {
  extern __shared__ __attribute__((aligned(16))) float depthwise_conv_lds[];
  float* xs = depthwise_conv_lds;                                 // [rows][stride]: frames t0 - P ... of xp
  float* gs = xs + kDwConvRows * a.stride;                        // [rows][kDwConvGradTile]: frames t0 ... of g
  const int tile = int(blockIdx.x % a.tiles_t), t0 = tile * kDwConvGradTile;
  const int64_t row0 = int64_t(blockIdx.x / a.tiles_t) * kDwConvRows;
  const int base = t0 + a.delta;
  const int a0 = base & ~3;
  const int s = base - a0;
  depthwise_conv_stage<VEC>(xs, a.stride, x, row0, a.rows, a.Lin, a0, (s + kDwConvGradTile + a.halo + 3) & ~3);
  depthwise_conv_stage<VEC>(gs, kDwConvGradTile, g, row0, a.rows, a.Lout, t0, kDwConvGradTile);
  __syncthreads();
  const int r = threadIdx.x / kDwConvRowLanes, l = threadIdx.x % kDwConvRowLanes;
  const int64_t row = row0 + r;
  const float* xr = xs + r * a.stride + l + s;
  double gv[kDwConvLaneFrames];
  bool has[kDwConvLaneFrames];                                    // frames past the row's end do not exist
#pragma unroll
  for (int m = 0; m < kDwConvLaneFrames; ++m) {
    const int i = l + m * kDwConvRowLanes;
    has[m] = t0 + i < a.Lout;
    gv[m] = double(gs[r * kDwConvGradTile + i]);
  }
  const int64_t b = row / a.C;
  const int c = int(row % a.C);
  double* dst = partial + ((b * a.tiles_t + tile) * a.C + c) * (a.K + 1);
  for (int k = k_begin; k < k_end; ++k) {
    double acc = 0.0;
    if (k < a.K) {
      const int off = a.off[k];
#pragma unroll
      for (int m = 0; m < kDwConvLaneFrames; ++m) {
        const double p = fma(gv[m], double(xr[m * kDwConvRowLanes + off]), acc);
        acc = has[m] ? p : acc;
      }
    } else {
#pragma unroll
      for (int m = 0; m < kDwConvLaneFrames; ++m) acc = has[m] ? acc + gv[m] : acc;
    }
#pragma unroll
    for (int d = kDwConvRowLanes / 2; d >= 1; d /= 2) acc += __shfl_xor(acc, d, kDwConvRowLanes);
    if (l == 0 && row < a.rows) dst[k] = acc;
  }
}

// grid: blocks of kDwConvFoldCols columns of the (C, K + 1) partials; the sums of one (channel, tap) pair, rounded to float32 once
__global__ __launch_bounds__(kDwConvThreads) void depthwise_conv_fold_kernel(const double* __restrict__ partial, int64_t n, int C, int K,
                                                                             float* __restrict__ dw /* NULL: not wanted */,
                                                                             float* __restrict__ db /* NULL: not wanted */) {
  __shared__ double segs[kDwConvFoldSegs][kDwConvFoldCols];
  const int col = threadIdx.x % kDwConvFoldCols, q = threadIdx.x / kDwConvFoldCols;
  const int64_t cols = int64_t(C) * (K + 1);
  const int64_t j = int64_t(blockIdx.x) * kDwConvFoldCols + col;
  const int k = int(j % (K + 1));
  const bool wanted = j < cols && (k < K ? dw != nullptr : db != nullptr);
  const int64_t len = depthwise_conv_fold_seg_len(n);
  const int64_t first = q * len, last = first + len < n ? first + len : n;
  double s = 0.0;
  if (wanted) {
#pragma unroll 8                                                  // (eight loads in flight; the additions keep their order)
    for (int64_t t = first; t < last; ++t) s += partial[t * cols + j];
  }
  segs[q][col] = s;
  __syncthreads();
  if (q != 0 || !wanted) return;
  const int nseg = int((n + len - 1) / len);                      // segments that hold a partial
  double sum = segs[0][col];
  for (int i = 1; i < nseg; ++i) sum += segs[i][col];
  const int64_t c = j / (K + 1);
  if (k < K) dw[c * K + k] = float(sum);
  else db[c] = float(sum);
}

}  // namespace wekws
