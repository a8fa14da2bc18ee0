// The host plan of the dense (groups 1) dilated Conv1d (dense_conv.hip.h): the arithmetic it states, the checks every call makes,
// the grids, the workspace and the LDS.  Pure host C++, no HIP.
//
// nn.Conv1d(Ci, Co, K, dilation=d) over x (B, Ci, Tin) with P zeros supplied in front of every row (0 <= P <= (K-1) d;
// Tout = Tin + P - (K-1) d; xp[n < 0] = 0) -- depthwise_conv_plan.h's convention: y and g (B, Co, Tout), float32, contiguous;
// w (Co, Ci, K) as nn.Conv1d holds it; bias (Co) or none.
//   forward  y[b][o][t]: acc = +0; for k ascending and, inside it, i ascending acc = fmaf(w[o][i][k], xp[b][i][t + k d - P], acc);
//            then one float32 addition of bias[o], none without a bias -- what v_mfma_f32_16x16x4_f32 computes from a zeroed
//            accumulator with the reduction index j = k Ci + i.  Padding a tap's channels up to the MFMA's 4 or to a stage puts
//            arithmetic zeros in both operands: fmaf(0, 0, acc) == acc, and an accumulator that started at +0 is never -0.  The
//            zeros of the left padding are real operands of one side only: an infinite weight over them is NaN, as in
//            F.conv1d(F.pad(x, (P, 0)), w).
//   dx       dx[b][i][n]: the same chain over k ascending and, inside it, o ascending,
//            acc = fmaf(w[o][i][k], g[b][o][n + P - k d], acc), g an arithmetic zero outside [0, Tout); no bias: the forward kernel
//            with the weight fetched transposed and the taps' shifts negated.  Non-finite weights are outside the contract here:
//            the reference has no terms where g does not exist.
//   dw, db   dw[:, :, k] obeys the contract of linear_wgrad_plan.h, unchanged, tap by tap, with rows r = b Tout + t, R = B Tout,
//            O = Co, I = Ci, g's row r = g[b][:, t] and x's row r of tap k = xp[b][:, t + k d - P]: chains of kWgradChain rows
//            counted from r = 0, slices added in double, the fold rounded once -- the bits of the row-major kernels on the
//            shifted, zero-padded, transposed copy, which is never made.  db is that contract's bias gradient, computed once.
// A (b, t) column of y and a (b, n) column of dx depend on batch row b alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "depthwise_conv_plan.h"
#include "pointwise_conv_plan.h"

namespace wekws {

constexpr int kDenseConvMaxTaps = kDwConvMaxTaps;      // K
constexpr int kDenseConvMaxWindow = kDwConvMaxWindow;  // (K-1) d + 1

inline int64_t dense_conv_tout(int64_t Tin, int64_t K, int64_t d, int64_t P) { return depthwise_conv_tout(Tin, K, d, P); }

// 0 fine, else the reason the shape is refused
inline const char* dense_conv_shape_check(int64_t B, int64_t Ci, int64_t Tin, int64_t Co, int64_t K, int64_t d, int64_t P) {
  if (B < 1 || B > INT32_MAX) return "B must be within 1 .. 2^31 - 1";
  if (Tin < 1 || Tin > INT32_MAX) return "Tin must be within 1 .. 2^31 - 1";
  if (Ci < 1 || Ci > kWgradMaxDim) return "Ci must be within 1 .. 65535";
  if (Co < 1 || Co > kWgradMaxDim) return "Co must be within 1 .. 65535";
  if (K < 1 || K > kDenseConvMaxTaps) return "K must be in 1..32";
  if (d < 1) return "dilation must be >= 1";
  if ((K - 1) * d + 1 > kDenseConvMaxWindow) return "a window above 256 frames";
  if (P < 0 || P > (K - 1) * d) return "left_pad must be in 0..(K-1)*dilation";
  if (dense_conv_tout(Tin, K, d, P) < 1) return "Tin + left_pad shorter than the window: no output frame";
  return nullptr;
}

// Everything below: arguments already checked by dense_conv_shape_check.
inline int64_t dense_conv_rows(int64_t B, int64_t Tout) { return B * Tout; }
// workgroups of the product that writes `channels` channels of `frames` frames: pointwise_conv_plan.h's (batch row, frame tile,
// channel tile); the forward writes (Co, Tout), dx (Ci, Tin)
inline int64_t dense_conv_grid(int64_t B, int64_t frames, int64_t channels) { return pointwise_conv_grid(B, frames, channels); }
inline int dense_conv_lds_bytes() { return pointwise_conv_lds_bytes(); }
// stages of a product over `channels` reduction channels: taps outermost, a tap's channel stages inside
inline int64_t dense_conv_stages(int64_t channels, int64_t K) { return K * wgrad_ceil_div(channels, kPwStage); }

// the workspace: per tap, linear_wgrad_plan.h's workspace of (R, Co, Ci); the bias rows of tap 0's are the only ones used
inline int64_t dense_conv_tap_workspace_bytes(int64_t B, int64_t Ci, int64_t Tout, int64_t Co) {
  return linear_wgrad_workspace_bytes(dense_conv_rows(B, Tout), Co, Ci);
}
inline int64_t dense_conv_workspace_bytes(int64_t B, int64_t Ci, int64_t Tout, int64_t Co, int64_t K) {
  return K * dense_conv_tap_workspace_bytes(B, Ci, Tout, Co);
}

// the grids of everything a shape may launch; taps are the second grid dimension of the partial and the fold launch
inline const char* dense_conv_grid_check(int64_t B, int64_t Ci, int64_t Tin, int64_t Co, int64_t K, int64_t d, int64_t P) {
  const int64_t Tout = dense_conv_tout(Tin, K, d, P), R = dense_conv_rows(B, Tout);
  if (dense_conv_grid(B, Tout, Co) > INT32_MAX || dense_conv_grid(B, Tin, Ci) > INT32_MAX || linear_wgrad_grid(R, Co, Ci) > INT32_MAX ||
      linear_wgrad_fold_grid(Co, Ci) > INT32_MAX)
    return "grid too large for one launch";
  return nullptr;
}

// 0 fine, else the reason the call is refused
inline const char* dense_conv_forward_check(const void* x, int64_t B, int64_t Ci, int64_t Tin, const void* w, int64_t Co, int64_t K,
                                            int64_t d, int64_t P, const void* y) {
  if (const char* why = dense_conv_shape_check(B, Ci, Tin, Co, K, d, P)) return why;
  if (const char* why = dense_conv_grid_check(B, Ci, Tin, Co, K, d, P)) return why;
  if (!x || !w || !y) return "x, w and y are needed";
  return nullptr;
}

inline const char* dense_conv_backward_check(const void* x, const void* grad_y, int64_t B, int64_t Ci, int64_t Tin, const void* w,
                                             int64_t Co, int64_t K, int64_t d, int64_t P, const void* grad_x, const void* grad_w,
                                             const void* grad_bias, const void* workspace, size_t workspace_bytes) {
  if (const char* why = dense_conv_shape_check(B, Ci, Tin, Co, K, d, P)) return why;
  if (const char* why = dense_conv_grid_check(B, Ci, Tin, Co, K, d, P)) return why;
  if (!grad_x && !grad_w && !grad_bias) return "none of grad_x, grad_w and grad_bias is wanted";
  if (!x || !grad_y || !w) return "x, grad_y and w are needed";
  if (grad_w || grad_bias) {
    if (!workspace) return "the workspace is needed";
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return "the workspace must be 16-byte aligned";
    if (workspace_bytes < size_t(dense_conv_workspace_bytes(B, Ci, dense_conv_tout(Tin, K, d, P), Co, K))) return "the workspace is too small";
  }
  return nullptr;
}

}  // namespace wekws
