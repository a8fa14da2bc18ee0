// The dense dilated Conv1d: launches and C entry points (kernels: dense_conv.hip.h and, for the weight and bias gradients,
// linear_wgrad.hip.h through linear_wgrad_launch_taps; the plan: dense_conv_plan.h).
#include "dense_conv.hip.h"

#include "host_util.h"

namespace {

// v (B, C, Tv) -> y (B, M, N); w (Co, Ci, taps) read as w[m][c][k], or as w[c][m][k] when TRANS; shift_k = shift0 + k shift_step
template <bool TRANS, bool BIAS>
bool launch_mm(const float* v, const float* w, const float* bias, float* y, int B, int C, int M, int Tv, int N, int taps, int shift0,
               int shift_step, int Ci, hipStream_t s) {
  const int tiles_m = int(wekws::wgrad_ceil_div(M, wekws::kPwTile)), tiles_n = int(wekws::wgrad_ceil_div(N, wekws::kPwTile));
  const dim3 grid(unsigned(wekws::dense_conv_grid(B, N, M))), block(wekws::kPwThreads);
  if (Tv % 4 == 0 && aligned16(v))
    hipLaunchKernelGGL((wekws::dense_conv_mm<TRANS, BIAS, true>), grid, block, 0, s, v, w, bias, y, C, M, Tv, N, taps, shift0, shift_step, Ci,
                       tiles_m, tiles_n);
  else
    hipLaunchKernelGGL((wekws::dense_conv_mm<TRANS, BIAS, false>), grid, block, 0, s, v, w, bias, y, C, M, Tv, N, taps, shift0, shift_step, Ci,
                       tiles_m, tiles_n);
  return hipGetLastError() == hipSuccess;
}

}  // namespace

#define DENSE_SHAPE_FMT "%s (B=%d Ci=%d Tin=%d Co=%d K=%d dilation=%d left_pad=%d)"

extern "C" {

int wekws_hip_dense_conv1d_plan(int B, int Ci, int Tin, int Co, int K, int dilation, int left_pad, int64_t out[10]) {
  if (!out) return fail(WEKWS_HIP_EINVAL, "dense_conv1d_plan: out is NULL");
  const char* why = wekws::dense_conv_shape_check(B, Ci, Tin, Co, K, dilation, left_pad);
  if (!why) why = wekws::dense_conv_grid_check(B, Ci, Tin, Co, K, dilation, left_pad);
  if (why) return fail(WEKWS_HIP_EINVAL, "dense_conv1d_plan: " DENSE_SHAPE_FMT, why, B, Ci, Tin, Co, K, dilation, left_pad);
  const int64_t Tout = wekws::dense_conv_tout(Tin, K, dilation, left_pad), R = wekws::dense_conv_rows(B, Tout);
  out[0] = wekws::kWgradChain;
  out[1] = wekws::linear_wgrad_chains(R);
  out[2] = wekws::linear_wgrad_slices(R, Co, Ci);
  out[3] = wekws::linear_wgrad_grid(R, Co, Ci);
  out[4] = wekws::dense_conv_workspace_bytes(B, Ci, Tout, Co, K);
  out[5] = wekws::dense_conv_grid(B, Tout, Co);
  out[6] = wekws::dense_conv_grid(B, Tin, Ci);
  out[7] = K;
  out[8] = wekws::linear_wgrad_fold_grid(Co, Ci);
  out[9] = Tout;
  return WEKWS_HIP_OK;
}

size_t wekws_hip_dense_conv1d_workspace_bytes(int B, int Ci, int Tin, int Co, int K, int dilation, int left_pad) {
  if (const char* why = wekws::dense_conv_shape_check(B, Ci, Tin, Co, K, dilation, left_pad)) {
    fail(WEKWS_HIP_EINVAL, "dense_conv1d_workspace_bytes: " DENSE_SHAPE_FMT, why, B, Ci, Tin, Co, K, dilation, left_pad);
    return 0;
  }
  return size_t(wekws::dense_conv_workspace_bytes(B, Ci, wekws::dense_conv_tout(Tin, K, dilation, left_pad), Co, K));
}

int wekws_hip_dense_conv1d_forward(const float* x, int B, int Ci, int Tin, const float* w, const float* bias, int Co, int K, int dilation,
                                   int left_pad, float* y, void* stream) {
  if (const char* why = wekws::dense_conv_forward_check(x, B, Ci, Tin, w, Co, K, dilation, left_pad, y))
    return fail(WEKWS_HIP_EINVAL, "dense_conv1d_forward: " DENSE_SHAPE_FMT, why, B, Ci, Tin, Co, K, dilation, left_pad);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int Tout = int(wekws::dense_conv_tout(Tin, K, dilation, left_pad));
  const bool ok = bias ? launch_mm<false, true>(x, w, bias, y, B, Ci, Co, Tin, Tout, K, -left_pad, dilation, Ci, s)
                       : launch_mm<false, false>(x, w, nullptr, y, B, Ci, Co, Tin, Tout, K, -left_pad, dilation, Ci, s);
  if (!ok) return fail(WEKWS_HIP_EDEVICE, "dense_conv1d_forward: the launch failed");
  return WEKWS_HIP_OK;
}

int wekws_hip_dense_conv1d_backward(const float* x, const float* grad_y, int B, int Ci, int Tin, const float* w, int Co, int K, int dilation,
                                    int left_pad, float* grad_x, float* grad_w, float* grad_bias, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (const char* why = wekws::dense_conv_backward_check(x, grad_y, B, Ci, Tin, w, Co, K, dilation, left_pad, grad_x, grad_w, grad_bias,
                                                         workspace, workspace_bytes))
    return fail(WEKWS_HIP_EINVAL, "dense_conv1d_backward: " DENSE_SHAPE_FMT, why, B, Ci, Tin, Co, K, dilation, left_pad);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int Tout = int(wekws::dense_conv_tout(Tin, K, dilation, left_pad));
  if (grad_x && !launch_mm<true, false>(grad_y, w, nullptr, grad_x, B, Co, Ci, Tout, Tin, K, left_pad, -dilation, Ci, s))
    return fail(WEKWS_HIP_EDEVICE, "dense_conv1d_backward: the grad_x launch failed");
  if (grad_w || grad_bias) {
    if (const char* why = wekws::linear_wgrad_launch_taps(x, grad_y, B, Tin, Tout, Co, Ci, K, dilation, left_pad, grad_w, grad_bias, workspace,
                                                          stream))
      return fail(WEKWS_HIP_EDEVICE, "dense_conv1d_backward: %s", why);
  }
  return WEKWS_HIP_OK;
}

}  // extern "C"
