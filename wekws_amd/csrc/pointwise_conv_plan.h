// The host plan of the pointwise (kernel_size 1) Conv1d (pointwise_conv.hip.h): the arithmetic it states, the checks every call
// makes, the grids and the LDS.  Pure host C++, no HIP.
//
// x (B, Ci, T), y and g (B, Co, T), float32, contiguous; w (Co, Ci), the (Co, Ci, 1) weight of nn.Conv1d; bias (Co) or none.
//   forward  y[b][o][t]: acc = +0; for i ascending acc = fmaf(w[o][i], x[b][i][t], acc); then one float32 addition of bias[o],
//            none without a bias -- what v_mfma_f32_16x16x4_f32 computes from a zeroed accumulator with k = i.  Padding i up to
//            the MFMA's 4 or to a stage puts arithmetic zeros in both operands: fmaf(0, 0, acc) == acc, and an accumulator that
//            started at +0 is never -0.
//   dx       dx[b][i][t]: the same chain over o ascending, fmaf(w[o][i], g[b][o][t], acc), no bias: the forward kernel with the
//            weight fetched transposed.
//   dw, db   the contract of linear_wgrad_plan.h, unchanged, with rows r = b T + t, R = B T, O = Co, I = Ci: chains of
//            kWgradChain rows counted from r = 0 (a chain may start or end inside a batch row), slices added in double, the
//            fold rounded once.  The slicing, workspace and grid functions are linear_wgrad_plan.h's own, so the bits are those of
//            the row-major kernels on x.transpose(1, 2).reshape(R, Ci) and g.transpose(1, 2).reshape(R, Co).
// A (b, t) column's forward and dx results depend on that column alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "linear_wgrad_plan.h"

namespace wekws {

constexpr int kPwTile = kWgradTile;        // a workgroup's tile of y is kPwTile channels x kPwTile frames of one batch row
constexpr int kPwThreads = kWgradThreads;  // 4 waves, each a 32 x 32 quadrant
constexpr int kPwStage = kWgradStage;      // reduction channels a stage brings to LDS
constexpr int kPwStride = kWgradStride;    // floats between two rows of an LDS stage

// 0 fine, else the reason the shape is refused
inline const char* pointwise_conv_shape_check(int64_t B, int64_t Ci, int64_t T, int64_t Co) {
  if (B < 1 || B > INT32_MAX) return "B must be within 1 .. 2^31 - 1";
  if (T < 1 || T > INT32_MAX) return "T must be within 1 .. 2^31 - 1";
  if (Ci < 1 || Ci > kWgradMaxDim) return "Ci must be within 1 .. 65535";
  if (Co < 1 || Co > kWgradMaxDim) return "Co must be within 1 .. 65535";
  return nullptr;
}

// Everything below: arguments already checked by pointwise_conv_shape_check.
inline int64_t pointwise_conv_rows(int64_t B, int64_t T) { return B * T; }
// workgroups of the product that writes `channels` output channels: (batch row, frame tile, channel tile), channel tile fastest
inline int64_t pointwise_conv_grid(int64_t B, int64_t T, int64_t channels) {
  return B * wgrad_ceil_div(T, kPwTile) * wgrad_ceil_div(channels, kPwTile);
}
// static LDS of the product kernel in bytes: two buffers of a weight stage and an x stage
inline int pointwise_conv_lds_bytes() { return 2 * 2 * kPwStage * kPwStride * int(sizeof(float)); }

inline int64_t pointwise_conv_workspace_bytes(int64_t B, int64_t Ci, int64_t T, int64_t Co) {
  return linear_wgrad_workspace_bytes(pointwise_conv_rows(B, T), Co, Ci);
}

// the grids of everything a shape may launch
inline const char* pointwise_conv_grid_check(int64_t B, int64_t Ci, int64_t T, int64_t Co) {
  const int64_t R = pointwise_conv_rows(B, T);
  if (pointwise_conv_grid(B, T, Co) > INT32_MAX || pointwise_conv_grid(B, T, Ci) > INT32_MAX ||
      linear_wgrad_grid(R, Co, Ci) > INT32_MAX || linear_wgrad_fold_grid(Co, Ci) > INT32_MAX)
    return "grid too large for one launch";
  return nullptr;
}

// 0 fine, else the reason the call is refused
inline const char* pointwise_conv_forward_check(const void* x, int64_t B, int64_t Ci, int64_t T, const void* w, int64_t Co,
                                                const void* y) {
  if (const char* why = pointwise_conv_shape_check(B, Ci, T, Co)) return why;
  if (const char* why = pointwise_conv_grid_check(B, Ci, T, Co)) return why;
  if (!x || !w || !y) return "x, w and y are needed";
  return nullptr;
}

inline const char* pointwise_conv_backward_check(const void* x, const void* grad_y, int64_t B, int64_t Ci, int64_t T, const void* w,
                                                 int64_t Co, const void* grad_x, const void* grad_w, const void* grad_bias,
                                                 const void* workspace, size_t workspace_bytes) {
  if (const char* why = pointwise_conv_shape_check(B, Ci, T, Co)) return why;
  if (const char* why = pointwise_conv_grid_check(B, Ci, T, Co)) return why;
  if (!grad_x && !grad_w && !grad_bias) return "none of grad_x, grad_w and grad_bias is wanted";
  if (!x || !grad_y || !w) return "x, grad_y and w are needed";
  if (grad_w || grad_bias) {
    if (!workspace) return "the workspace is needed";
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return "the workspace must be 16-byte aligned";
    if (workspace_bytes < size_t(pointwise_conv_workspace_bytes(B, Ci, T, Co))) return "the workspace is too small";
  }
  return nullptr;
}

}  // namespace wekws
