// The host plan of the trainable BatchNorm1d (batchnorm.hip.h): rows a workgroup, frames a tile, the fold of the partial sums,
// the workspace layout and the checks every call makes.  Pure host C++, no HIP.
//
// nn.BatchNorm1d over a (B, C, T) tensor, N = B T values a channel, with the ReLU and the residual add that follow it in the
// reference's blocks (DsCnnBlock.cnn[1:3] / [4:6], DSDilatedConv1d.bn, TCNBlock.bn1 / relu1, TCNBlock.bn2 + inputs + relu2):
//     batch statistics:  mean = sum x / N,  var = sum (x - mean)^2 / N,  invstd = 1 / sqrt(var + eps)
//     running buffers:   mean = running_mean,  invstd = 1 / sqrt(running_var + eps)
//     z = (x - mean) invstd weight + bias (+ residual),  y = relu(z) or z
// Time is the contiguous axis, so a row is one (b, c) pair and the lanes of a wave run along t (depthwise_conv_plan.h).
#pragma once
#include <stdint.h>

namespace wekws {

constexpr int kBnThreads = 256;                      // lanes of a workgroup of every kernel
constexpr int kBnRows = 8;                           // (b, c) rows a workgroup owns: 32 lanes along t each
constexpr int kBnRowLanes = kBnThreads / kBnRows;
constexpr int kBnLaneFrames = 4;                     // consecutive frames a lane owns: one 16-byte access
constexpr int kBnTile = kBnRowLanes * kBnLaneFrames; // 128 frames of a row a workgroup owns: one partial each
constexpr int kBnFoldSegs = 8;                       // the fold: up to 8 segments of consecutive partials, then the segments' sums
constexpr int kBnFoldChans = kBnThreads / kBnFoldSegs;   // channels a workgroup of the fold owns

inline int64_t batchnorm_row_blocks(int64_t B, int64_t C) { return (B * C + kBnRows - 1) / kBnRows; }
inline int64_t batchnorm_tiles_t(int64_t T) { return (T + kBnTile - 1) / kBnTile; }
// workgroups of the partial-sum and of the elementwise kernels
inline int64_t batchnorm_tiles(int64_t B, int64_t C, int64_t T) { return batchnorm_row_blocks(B, C) * batchnorm_tiles_t(T); }
// partial sums a channel has: one pair per batch row and frame tile
inline int64_t batchnorm_partials(int64_t B, int64_t T) { return B * batchnorm_tiles_t(T); }
// the fold of `n` partials: segments of this many consecutive partials (at most kBnFoldSegs of them) are summed in ascending
// order, then the segments' sums in ascending segment order -- a function of the count alone (constexpr: the kernel calls it)
constexpr int64_t batchnorm_fold_seg_len(int64_t n) { return (n + kBnFoldSegs - 1) / kBnFoldSegs; }

// 0 fine, else the reason the shape is refused
inline const char* batchnorm_check(int64_t B, int64_t C, int64_t T) {
  if (B < 1 || C < 1 || T < 1) return "B, C and T must be >= 1";
  if (B > INT32_MAX || C > INT32_MAX || T > INT32_MAX) return "B, C or T too large for one launch";
  if (batchnorm_tiles(B, C, T) > INT32_MAX) return "B * C * T too large for one launch";
  return nullptr;
}

// Workspace, every part a multiple of 16 bytes:
//   [0, partial_bytes)      (partials, C, 2) doubles: forward sum (x - shift), sum (x - shift)^2; backward sum g', sum g' (x - mean)
//   then (C, 2) floats      backward with batch statistics: sum g' / N and invstd^2 sum g' (x - mean) / N, as the grad_x kernel reads them
//   then 16 bytes           forward: num_batches_tracked as it was before the call
inline int64_t batchnorm_partial_bytes(int64_t B, int64_t C, int64_t T) {
  return (batchnorm_partials(B, T) * C * 2 * int64_t(sizeof(double)) + 15) / 16 * 16;
}
inline int64_t batchnorm_coef_bytes(int64_t C) { return (C * 2 * int64_t(sizeof(float)) + 15) / 16 * 16; }
inline int64_t batchnorm_workspace_bytes(int64_t B, int64_t C, int64_t T) {
  return batchnorm_partial_bytes(B, C, T) + batchnorm_coef_bytes(C) + 16;
}
// static LDS of the fold kernel, in bytes: two sums a (segment, channel); the other kernels use none
constexpr int kBnFoldLdsBytes = 2 * kBnFoldSegs * kBnFoldChans * int(sizeof(double));

}  // namespace wekws
