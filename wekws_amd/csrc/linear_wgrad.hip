// The Linear layers' weight and bias gradients: launches and C entry points (kernels: linear_wgrad.hip.h; the plan:
// linear_wgrad_plan.h).
#include "linear_wgrad.hip.h"

#include "host_util.h"

namespace {

// the taps of a dense Conv1d (TAP): the second grid dimension of the partial launch
struct Taps {
  int taps = 1, dil = 0, pad = 0;
  int64_t Tx = 0, stride = 0;                   // frames of a batch row of x; doubles between two taps' partials
};

template <bool VEC, bool BCT, bool TAP = false>
bool launch_partial(const float* x, const float* g, int64_t R, int O, int I, int64_t T, bool want_w, double* ws_w, double* ws_b,
                    hipStream_t s, const Taps& t = Taps()) {
  const int64_t grid = want_w ? wekws::linear_wgrad_grid(R, O, I) : wekws::linear_wgrad_bias_grid(R, O, I);
  const int tiles_i = want_w ? int(wekws::wgrad_ceil_div(I, wekws::kWgradTile)) : 1;
  hipLaunchKernelGGL((wekws::linear_wgrad_partial<VEC, BCT, TAP>), dim3(unsigned(grid), unsigned(want_w ? t.taps : 1)),
                     dim3(wekws::kWgradThreads), 0, s, x, g, R, O, I, tiles_i, wekws::linear_wgrad_chains_per_slice(R, O, I),
                     wekws::linear_wgrad_padded(O), wekws::linear_wgrad_padded(I), want_w ? ws_w : nullptr, ws_b, T, t.Tx, t.dil, t.pad,
                     t.stride);
  return hipGetLastError() == hipSuccess;
}

// the fold of `taps` taps whose partials lie tap_stride doubles apart, for arguments already checked
const char* launch_fold(double* ws, int64_t R, int O, int I, float* grad_w, float* grad_bias, int taps, int64_t tap_stride, hipStream_t s) {
  const int64_t n_w = int64_t(O) * I;
  const int64_t first = grad_w ? 0 : n_w, last = grad_bias ? n_w + O : n_w;
  hipLaunchKernelGGL(wekws::linear_wgrad_fold, dim3(unsigned(wekws::wgrad_ceil_div(last - first, wekws::kWgradFoldThreads)),
                                                    unsigned(grad_w ? taps : 1)),
                     dim3(wekws::kWgradFoldThreads), 0, s, ws, O, I, wekws::linear_wgrad_slices(R, O, I), wekws::linear_wgrad_padded(O),
                     wekws::linear_wgrad_padded(I), wekws::linear_wgrad_bias_offset(R, O, I), first, last, grad_w, grad_bias, tap_stride);
  return hipGetLastError() == hipSuccess ? nullptr : "the fold launch failed";
}

}  // namespace

namespace wekws {

const char* linear_wgrad_launch(const float* x, const float* g, int64_t R, int O, int I, int64_t frames, float* grad_w, float* grad_bias,
                                void* workspace, void* stream) {
  const hipStream_t s = static_cast<hipStream_t>(stream);
  double* const ws = static_cast<double*>(workspace);
  const int64_t bias_offset = linear_wgrad_bias_offset(R, O, I);
  double* const ws_b = grad_bias ? ws + bias_offset : nullptr;
  const bool want_w = grad_w != nullptr;
  bool ok;
  if (frames > 0) {
    const bool vec = frames % 4 == 0 && aligned16(x) && aligned16(g);
    ok = vec ? launch_partial<true, true>(x, g, R, O, I, frames, want_w, ws, ws_b, s)
             : launch_partial<false, true>(x, g, R, O, I, frames, want_w, ws, ws_b, s);
  } else {
    const bool vec = O % 4 == 0 && I % 4 == 0 && aligned16(x) && aligned16(g);
    ok = vec ? launch_partial<true, false>(x, g, R, O, I, 0, want_w, ws, ws_b, s)
             : launch_partial<false, false>(x, g, R, O, I, 0, want_w, ws, ws_b, s);
  }
  if (!ok) return "the partial launch failed";
  return launch_fold(ws, R, O, I, grad_w, grad_bias, 1, 0, s);
}

const char* linear_wgrad_launch_taps(const float* x, const float* g, int64_t B, int64_t Tin, int64_t Tout, int O, int I, int K, int dilation,
                                     int left_pad, float* grad_w, float* grad_bias, void* workspace, void* stream) {
  const hipStream_t s = static_cast<hipStream_t>(stream);
  double* const ws = static_cast<double*>(workspace);
  const int64_t R = B * Tout;
  double* const ws_b = grad_bias ? ws + linear_wgrad_bias_offset(R, O, I) : nullptr;
  Taps t;
  t.taps = K, t.dil = dilation, t.pad = left_pad, t.Tx = Tin;
  t.stride = linear_wgrad_workspace_bytes(R, O, I) / int64_t(sizeof(double));
  const bool vec = Tout % 4 == 0 && aligned16(g);               // of the g fetch; a tap's x fetch is scalar
  const bool ok = vec ? launch_partial<true, true, true>(x, g, R, O, I, Tout, grad_w != nullptr, ws, ws_b, s, t)
                      : launch_partial<false, true, true>(x, g, R, O, I, Tout, grad_w != nullptr, ws, ws_b, s, t);
  if (!ok) return "the partial launch failed";
  return launch_fold(ws, R, O, I, grad_w, grad_bias, K, t.stride, s);
}

}  // namespace wekws

extern "C" {

int wekws_hip_linear_wgrad_plan(int64_t R, int O, int I, int64_t out[5]) {
  if (!out) return fail(WEKWS_HIP_EINVAL, "linear_wgrad_plan: out is NULL");
  if (const char* why = wekws::linear_wgrad_shape_check(R, O, I))
    return fail(WEKWS_HIP_EINVAL, "linear_wgrad_plan: %s (R=%lld O=%d I=%d)", why, static_cast<long long>(R), O, I);
  if (wekws::linear_wgrad_grid(R, O, I) > INT32_MAX) return fail(WEKWS_HIP_EINVAL, "linear_wgrad_plan: grid too large for one launch");
  out[0] = wekws::kWgradChain;
  out[1] = wekws::linear_wgrad_chains(R);
  out[2] = wekws::linear_wgrad_slices(R, O, I);
  out[3] = wekws::linear_wgrad_grid(R, O, I);
  out[4] = wekws::linear_wgrad_workspace_bytes(R, O, I);
  return WEKWS_HIP_OK;
}

size_t wekws_hip_linear_wgrad_workspace_bytes(int64_t R, int O, int I) {
  if (const char* why = wekws::linear_wgrad_shape_check(R, O, I)) {
    fail(WEKWS_HIP_EINVAL, "linear_wgrad_workspace_bytes: %s (R=%lld O=%d I=%d)", why, static_cast<long long>(R), O, I);
    return 0;
  }
  return size_t(wekws::linear_wgrad_workspace_bytes(R, O, I));
}

int wekws_hip_linear_wgrad(const float* x, const float* g, int64_t R, int O, int I, float* grad_w, float* grad_bias, void* workspace,
                           size_t workspace_bytes, void* stream) {
  if (const char* why = wekws::linear_wgrad_check(x, g, R, O, I, grad_w, grad_bias, workspace, workspace_bytes))
    return fail(WEKWS_HIP_EINVAL, "linear_wgrad: %s (R=%lld O=%d I=%d)", why, static_cast<long long>(R), O, I);
  if (const char* why = wekws::linear_wgrad_launch(x, g, R, O, I, 0, grad_w, grad_bias, workspace, stream))
    return fail(WEKWS_HIP_EDEVICE, "linear_wgrad: %s", why);
  return WEKWS_HIP_OK;
}

}  // extern "C"
