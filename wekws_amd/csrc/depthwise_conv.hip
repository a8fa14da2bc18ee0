// The trainable depthwise Conv1d: launches and C entry points (kernels: depthwise_conv.hip.h; the plan: depthwise_conv_plan.h).
#include "depthwise_conv.hip.h"

#include "host_util.h"

namespace {

using wekws::DepthwiseConvArgs;

// the shape and the tap table as the kernels read them.  sign +1: a tile's LDS columns start P frames before it and a tap
// reads halo - delay columns on (forward, tap gradient); -1: they start P - halo frames after it and a tap reads delay columns
// on (the input gradient, which reads rows of Tout frames and writes rows of Tin)
DepthwiseConvArgs make_args(int B, int C, int Tin, int K, int d, int P, int sign, int tile) {
  wekws::FsmnMemTap taps[wekws::kDwConvMaxTaps];
  const int Tout = int(wekws::depthwise_conv_tout(Tin, K, d, P));
  DepthwiseConvArgs a{};
  a.rows = int64_t(B) * C;
  a.C = C;
  a.K = wekws::depthwise_conv_taps(K, d, taps);
  a.halo = wekws::depthwise_conv_window(K, d) - 1;
  a.Lin = sign > 0 ? Tin : Tout;
  a.Lout = sign > 0 ? Tout : Tin;
  a.delta = sign > 0 ? -P : P - a.halo;
  a.tiles_t = (a.Lout + tile - 1) / tile;
  a.stride = wekws::depthwise_conv_stage_stride(tile, a.halo + 1);
  for (int k = 0; k < a.K; ++k) a.off[k] = int16_t(sign > 0 ? a.halo - taps[k].delay : taps[k].delay);
  return a;
}

// 16-byte accesses where every row of both tensors starts on a 16-byte boundary
bool can_vec(int Tin, int Tout, const void* p, const void* q) { return Tin % 4 == 0 && Tout % 4 == 0 && aligned16(p) && aligned16(q); }

template <bool BWD>
int launch_fir(const float* in, float* out, int B, const float* w, const float* bias, const DepthwiseConvArgs& a, hipStream_t s) {
  const dim3 grid(unsigned(wekws::depthwise_conv_fir_tiles(B, a.C, a.Lout)));
  const size_t lds = size_t(wekws::depthwise_conv_fir_lds_bytes(a.halo + 1));
  if (can_vec(a.Lin, a.Lout, in, out))
    hipLaunchKernelGGL((wekws::depthwise_conv_fir_kernel<4, BWD>), grid, dim3(wekws::kDwConvThreads), lds, s, in, out, w, bias, a);
  else
    hipLaunchKernelGGL((wekws::depthwise_conv_fir_kernel<1, BWD>), grid, dim3(wekws::kDwConvThreads), lds, s, in, out, w, bias, a);
  return hipGetLastError() != hipSuccess;
}

int check_shape(const char* what, int B, int C, int Tin, int K, int d, int P) {
  if (const char* why = wekws::depthwise_conv_check(B, C, Tin, K, d, P))
    return fail(WEKWS_HIP_EINVAL, "%s: %s (B=%d C=%d Tin=%d K=%d dilation=%d left_pad=%d)", what, why, B, C, Tin, K, d, P);
  return WEKWS_HIP_OK;
}

}  // namespace

extern "C" {

size_t wekws_hip_depthwise_conv1d_workspace_bytes(int B, int C, int Tin, int K, int dilation, int left_pad) {
  if (check_shape("depthwise_conv1d_workspace_bytes", B, C, Tin, K, dilation, left_pad)) return 0;
  return size_t(wekws::depthwise_conv_workspace_bytes(B, C, wekws::depthwise_conv_tout(Tin, K, dilation, left_pad), K));
}

int wekws_hip_depthwise_conv1d_forward(const float* x, int B, int C, int Tin, const float* w, const float* bias, int K, int dilation,
                                       int left_pad, float* y, void* stream) {
  if (!x || !w || !y) return fail(WEKWS_HIP_EINVAL, "depthwise_conv1d_forward: NULL argument");
  if (const int rc = check_shape("depthwise_conv1d_forward", B, C, Tin, K, dilation, left_pad)) return rc;
  const DepthwiseConvArgs a = make_args(B, C, Tin, K, dilation, left_pad, +1, wekws::kDwConvFirTile);
  if (launch_fir<false>(x, y, B, w, bias, a, static_cast<hipStream_t>(stream)))
    return fail(WEKWS_HIP_EDEVICE, "depthwise_conv1d_forward launch failed");
  return WEKWS_HIP_OK;
}

int wekws_hip_depthwise_conv1d_backward(const float* x, const float* grad_y, int B, int C, int Tin, const float* w, int K, int dilation,
                                        int left_pad, float* grad_x, float* grad_w, float* grad_bias, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  if (!x || !grad_y || !w) return fail(WEKWS_HIP_EINVAL, "depthwise_conv1d_backward: NULL argument");
  if (const int rc = check_shape("depthwise_conv1d_backward", B, C, Tin, K, dilation, left_pad)) return rc;
  const int Tout = int(wekws::depthwise_conv_tout(Tin, K, dilation, left_pad));
  if (grad_w || grad_bias)                                          // the tap and bias gradients' partial sums
    if (const int rc = check_workspace("depthwise_conv1d_backward", workspace, workspace_bytes,
                                       size_t(wekws::depthwise_conv_workspace_bytes(B, C, Tout, K)),
                                       "wekws_hip_depthwise_conv1d_workspace_bytes"))
      return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  bool bad = false;
  if (grad_x) {
    const DepthwiseConvArgs a = make_args(B, C, Tin, K, dilation, left_pad, -1, wekws::kDwConvFirTile);
    bad = launch_fir<true>(grad_y, grad_x, B, w, nullptr, a, s) != 0;
  }
  if (!bad && (grad_w || grad_bias)) {
    const DepthwiseConvArgs a = make_args(B, C, Tin, K, dilation, left_pad, +1, wekws::kDwConvGradTile);
    const dim3 grid(unsigned(wekws::depthwise_conv_grad_tiles(B, C, Tout)));
    const size_t lds = size_t(wekws::depthwise_conv_grad_lds_bytes(a.halo + 1));
    const int k_begin = grad_w ? 0 : K, k_end = grad_bias ? K + 1 : K;
    double* ws = static_cast<double*>(workspace);
    if (can_vec(Tin, Tout, x, grad_y))
      hipLaunchKernelGGL((wekws::depthwise_conv_tap_grad_kernel<4>), grid, dim3(wekws::kDwConvThreads), lds, s, x, grad_y, ws, a, k_begin,
                         k_end);
    else
      hipLaunchKernelGGL((wekws::depthwise_conv_tap_grad_kernel<1>), grid, dim3(wekws::kDwConvThreads), lds, s, x, grad_y, ws, a, k_begin,
                         k_end);
    bad = hipGetLastError() != hipSuccess;
    if (!bad) {
      const int64_t cols = int64_t(C) * (K + 1);
      hipLaunchKernelGGL(wekws::depthwise_conv_fold_kernel, dim3(unsigned((cols + wekws::kDwConvFoldCols - 1) / wekws::kDwConvFoldCols)),
                         dim3(wekws::kDwConvThreads), 0, s, static_cast<const double*>(ws), wekws::depthwise_conv_partials(B, Tout), C, K,
                         grad_w, grad_bias);
      bad = hipGetLastError() != hipSuccess;
    }
  }
  if (bad) return fail(WEKWS_HIP_EDEVICE, "depthwise_conv1d_backward launch failed");
  return WEKWS_HIP_OK;
}

}  // extern "C"
