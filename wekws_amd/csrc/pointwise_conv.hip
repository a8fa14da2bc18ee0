// The pointwise Conv1d: launches and C entry points (kernels: pointwise_conv.hip.h and, for the weight and bias gradients,
// linear_wgrad.hip.h through linear_wgrad_launch; the plan: pointwise_conv_plan.h).
#include "pointwise_conv.hip.h"

#include "host_util.h"

namespace {

template <bool TRANS, bool BIAS, bool VECX, bool VECW>
bool launch_mm4(const float* x, const float* w, const float* bias, float* y, int B, int K, int M, int T, int ldw, hipStream_t s) {
  const int tiles_m = int(wekws::wgrad_ceil_div(M, wekws::kPwTile)), tiles_t = int(wekws::wgrad_ceil_div(T, wekws::kPwTile));
  hipLaunchKernelGGL((wekws::pointwise_conv_mm<TRANS, BIAS, VECX, VECW>), dim3(unsigned(wekws::pointwise_conv_grid(B, T, M))),
                     dim3(wekws::kPwThreads), 0, s, x, w, bias, y, K, M, T, tiles_m, tiles_t, ldw);
  return hipGetLastError() == hipSuccess;
}

// x (B, K, T) -> y (B, M, T); w (Co, Ci) read as w[m][k], or as w[k][m] when TRANS; ldw = Ci
template <bool TRANS, bool BIAS>
bool launch_mm(const float* x, const float* w, const float* bias, float* y, int B, int K, int M, int T, int ldw, hipStream_t s) {
  const bool vx = T % 4 == 0 && aligned16(x), vw = ldw % 4 == 0 && aligned16(w);
  if (vx) return vw ? launch_mm4<TRANS, BIAS, true, true>(x, w, bias, y, B, K, M, T, ldw, s)
                    : launch_mm4<TRANS, BIAS, true, false>(x, w, bias, y, B, K, M, T, ldw, s);
  return vw ? launch_mm4<TRANS, BIAS, false, true>(x, w, bias, y, B, K, M, T, ldw, s)
            : launch_mm4<TRANS, BIAS, false, false>(x, w, bias, y, B, K, M, T, ldw, s);
}

}  // namespace

extern "C" {

int wekws_hip_pointwise_conv1d_plan(int B, int Ci, int T, int Co, int64_t out[7]) {
  if (!out) return fail(WEKWS_HIP_EINVAL, "pointwise_conv1d_plan: out is NULL");
  const char* why = wekws::pointwise_conv_shape_check(B, Ci, T, Co);
  if (!why) why = wekws::pointwise_conv_grid_check(B, Ci, T, Co);
  if (why) return fail(WEKWS_HIP_EINVAL, "pointwise_conv1d_plan: %s (B=%d Ci=%d T=%d Co=%d)", why, B, Ci, T, Co);
  const int64_t R = wekws::pointwise_conv_rows(B, T);
  out[0] = wekws::kWgradChain;
  out[1] = wekws::linear_wgrad_chains(R);
  out[2] = wekws::linear_wgrad_slices(R, Co, Ci);
  out[3] = wekws::linear_wgrad_grid(R, Co, Ci);
  out[4] = wekws::pointwise_conv_workspace_bytes(B, Ci, T, Co);
  out[5] = wekws::pointwise_conv_grid(B, T, Co);
  out[6] = wekws::pointwise_conv_grid(B, T, Ci);
  return WEKWS_HIP_OK;
}

size_t wekws_hip_pointwise_conv1d_workspace_bytes(int B, int Ci, int T, int Co) {
  if (const char* why = wekws::pointwise_conv_shape_check(B, Ci, T, Co)) {
    fail(WEKWS_HIP_EINVAL, "pointwise_conv1d_workspace_bytes: %s (B=%d Ci=%d T=%d Co=%d)", why, B, Ci, T, Co);
    return 0;
  }
  return size_t(wekws::pointwise_conv_workspace_bytes(B, Ci, T, Co));
}

int wekws_hip_pointwise_conv1d_forward(const float* x, int B, int Ci, int T, const float* w, const float* bias, int Co, float* y,
                                       void* stream) {
  if (const char* why = wekws::pointwise_conv_forward_check(x, B, Ci, T, w, Co, y))
    return fail(WEKWS_HIP_EINVAL, "pointwise_conv1d_forward: %s (B=%d Ci=%d T=%d Co=%d)", why, B, Ci, T, Co);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const bool ok = bias ? launch_mm<false, true>(x, w, bias, y, B, Ci, Co, T, Ci, s)
                       : launch_mm<false, false>(x, w, nullptr, y, B, Ci, Co, T, Ci, s);
  if (!ok) return fail(WEKWS_HIP_EDEVICE, "pointwise_conv1d_forward: the launch failed");
  return WEKWS_HIP_OK;
}

int wekws_hip_pointwise_conv1d_backward(const float* x, const float* grad_y, int B, int Ci, int T, const float* w, int Co, float* grad_x,
                                        float* grad_w, float* grad_bias, void* workspace, size_t workspace_bytes, void* stream) {
  if (const char* why = wekws::pointwise_conv_backward_check(x, grad_y, B, Ci, T, w, Co, grad_x, grad_w, grad_bias, workspace,
                                                             workspace_bytes))
    return fail(WEKWS_HIP_EINVAL, "pointwise_conv1d_backward: %s (B=%d Ci=%d T=%d Co=%d)", why, B, Ci, T, Co);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (grad_x && !launch_mm<true, false>(grad_y, w, nullptr, grad_x, B, Co, Ci, T, Ci, s))
    return fail(WEKWS_HIP_EDEVICE, "pointwise_conv1d_backward: the grad_x launch failed");
  if (grad_w || grad_bias) {
    if (const char* why = wekws::linear_wgrad_launch(x, grad_y, wekws::pointwise_conv_rows(B, T), Co, Ci, T, grad_w, grad_bias, workspace,
                                                     stream))
      return fail(WEKWS_HIP_EDEVICE, "pointwise_conv1d_backward: %s", why);
  }
  return WEKWS_HIP_OK;
}

}  // extern "C"
