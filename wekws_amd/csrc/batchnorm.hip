// The trainable BatchNorm1d: launches and C entry points (kernels: batchnorm.hip.h; the plan: batchnorm_plan.h).
#include "batchnorm.hip.h"

#include "host_util.h"

namespace {

using wekws::BatchNormArgs;

BatchNormArgs make_args(int B, int C, int T) {
  BatchNormArgs a{};
  a.rows = int64_t(B) * C;
  a.C = C;
  a.T = T;
  a.tiles_t = int(wekws::batchnorm_tiles_t(T));
  return a;
}

int check_shape(const char* what, int B, int C, int T, int batch_stats) {
  if (const char* why = wekws::batchnorm_check(B, C, T)) return fail(WEKWS_HIP_EINVAL, "%s: %s (B=%d C=%d T=%d)", what, why, B, C, T);
  if (batch_stats && int64_t(B) * T < 2)
    return fail(WEKWS_HIP_EINVAL, "%s: batch statistics need more than one value per channel (B=%d T=%d)", what, B, T);
  return WEKWS_HIP_OK;
}

int check_bn_workspace(const char* what, int B, int C, int T, const void* workspace, size_t workspace_bytes) {
  return check_workspace(what, workspace, workspace_bytes, size_t(wekws::batchnorm_workspace_bytes(B, C, T)),
                         "wekws_hip_batchnorm_workspace_bytes");
}

// the parts of the workspace (batchnorm_plan.h)
double* ws_partial(void* ws) { return static_cast<double*>(ws); }
float* ws_coef(void* ws, int B, int C, int T) { return reinterpret_cast<float*>(static_cast<char*>(ws) + wekws::batchnorm_partial_bytes(B, C, T)); }
int64_t* ws_tracked(void* ws, int B, int C, int T) {
  return reinterpret_cast<int64_t*>(static_cast<char*>(ws) + wekws::batchnorm_partial_bytes(B, C, T) + wekws::batchnorm_coef_bytes(C));
}

template <int VEC, bool RELU, bool RES>
void launch_apply(bool eval, dim3 grid, hipStream_t s, const float* x, const float* residual, float* y, const float* weight,
                  const float* bias, const float* rm, const float* rv, double eps, float* save_mean, float* save_invstd,
                  const BatchNormArgs& a) {
  const dim3 block(wekws::kBnThreads);
  if (eval)
    hipLaunchKernelGGL((wekws::batchnorm_apply_kernel<VEC, RELU, RES, true>), grid, block, 0, s, x, residual, y, weight, bias, rm, rv, eps,
                       save_mean, save_invstd, a);
  else
    hipLaunchKernelGGL((wekws::batchnorm_apply_kernel<VEC, RELU, RES, false>), grid, block, 0, s, x, residual, y, weight, bias, rm, rv, eps,
                       save_mean, save_invstd, a);
}

template <int VEC, typename... Args>
void launch_apply_flags(bool relu, bool res, Args... args) {
  if (relu && res) launch_apply<VEC, true, true>(args...);
  else if (relu) launch_apply<VEC, true, false>(args...);
  else if (res) launch_apply<VEC, false, true>(args...);
  else launch_apply<VEC, false, false>(args...);
}

template <int VEC, bool RELU>
void launch_grad_x(bool batch, dim3 grid, hipStream_t s, const float* x, const float* y, const float* g, const float* weight,
                   const float* save_mean, const float* save_invstd, const float* coef, float* dx, float* dres, const BatchNormArgs& a) {
  const dim3 block(wekws::kBnThreads);
  if (batch)
    hipLaunchKernelGGL((wekws::batchnorm_grad_x_kernel<VEC, RELU, true>), grid, block, 0, s, x, y, g, weight, save_mean, save_invstd, coef, dx,
                       dres, a);
  else
    hipLaunchKernelGGL((wekws::batchnorm_grad_x_kernel<VEC, RELU, false>), grid, block, 0, s, x, y, g, weight, save_mean, save_invstd, coef, dx,
                       dres, a);
}

}  // namespace

extern "C" {

size_t wekws_hip_batchnorm_workspace_bytes(int B, int C, int T) {
  if (check_shape("batchnorm_workspace_bytes", B, C, T, 0)) return 0;
  return size_t(wekws::batchnorm_workspace_bytes(B, C, T));
}

int wekws_hip_batchnorm_forward(const float* x, const float* residual, int B, int C, int T, const float* weight, const float* bias,
                                float* running_mean, float* running_var, int64_t* num_batches_tracked, int batch_stats, double momentum,
                                double eps, int relu, float* y, float* save_mean, float* save_invstd, void* workspace,
                                size_t workspace_bytes, void* stream) {
  const char* what = "batchnorm_forward";
  if (!x || !y || !save_mean || !save_invstd) return fail(WEKWS_HIP_EINVAL, "%s: NULL argument", what);
  if (const int rc = check_shape(what, B, C, T, batch_stats)) return rc;
  if (!(eps > 0.0)) return fail(WEKWS_HIP_EINVAL, "%s: eps must be > 0, got %g", what, eps);
  if (!(momentum <= 1.0)) return fail(WEKWS_HIP_EINVAL, "%s: momentum must be <= 1 (< 0: cumulative), got %g", what, momentum);
  if ((running_mean == nullptr) != (running_var == nullptr))
    return fail(WEKWS_HIP_EINVAL, "%s: running_mean and running_var: both or neither", what);
  if (!batch_stats && !running_mean) return fail(WEKWS_HIP_EINVAL, "%s: statistics from the running buffers, and no running buffers", what);
  if (batch_stats && running_mean && momentum < 0.0 && !num_batches_tracked)
    return fail(WEKWS_HIP_EINVAL, "%s: a cumulative average needs num_batches_tracked", what);
  if (batch_stats)
    if (const int rc = check_bn_workspace(what, B, C, T, workspace, workspace_bytes)) return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const BatchNormArgs a = make_args(B, C, T);
  const dim3 grid(unsigned(wekws::batchnorm_tiles(B, C, T))), block(wekws::kBnThreads);
  const bool vec = T % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(residual);
  if (batch_stats) {
    // the running buffers and the count move only where there are running buffers
    int64_t* tracked = running_mean ? num_batches_tracked : nullptr;
    int64_t* before = ws_tracked(workspace, B, C, T);
    if (T % 4 == 0 && aligned16(x))
      hipLaunchKernelGGL((wekws::batchnorm_stats_kernel<4>), grid, block, 0, s, x, ws_partial(workspace), tracked, before, a);
    else
      hipLaunchKernelGGL((wekws::batchnorm_stats_kernel<1>), grid, block, 0, s, x, ws_partial(workspace), tracked, before, a);
    if (hipGetLastError() != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "%s: launch failed", what);
    hipLaunchKernelGGL(wekws::batchnorm_stats_fold_kernel, dim3(unsigned((C + wekws::kBnFoldChans - 1) / wekws::kBnFoldChans)), block, 0, s,
                       static_cast<const double*>(ws_partial(workspace)), wekws::batchnorm_partials(B, T), x, C, T, double(int64_t(B) * T), eps,
                       momentum, running_mean, running_var, tracked, static_cast<const int64_t*>(before), save_mean, save_invstd);
    if (hipGetLastError() != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "%s: launch failed", what);
  }
  if (vec)
    launch_apply_flags<4>(relu != 0, residual != nullptr, !batch_stats, grid, s, x, residual, y, weight, bias, running_mean, running_var, eps,
                          save_mean, save_invstd, a);
  else
    launch_apply_flags<1>(relu != 0, residual != nullptr, !batch_stats, grid, s, x, residual, y, weight, bias, running_mean, running_var, eps,
                          save_mean, save_invstd, a);
  if (hipGetLastError() != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "%s: launch failed", what);
  return WEKWS_HIP_OK;
}

int wekws_hip_batchnorm_backward(const float* x, const float* y, const float* grad_y, int B, int C, int T, const float* weight,
                                 const float* save_mean, const float* save_invstd, int batch_stats, int relu, float* grad_x,
                                 float* grad_residual, float* grad_weight, float* grad_bias, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  const char* what = "batchnorm_backward";
  if (!x || !grad_y || !save_mean || !save_invstd) return fail(WEKWS_HIP_EINVAL, "%s: NULL argument", what);
  if (relu && !y) return fail(WEKWS_HIP_EINVAL, "%s: the ReLU's backward needs y", what);
  if (const int rc = check_shape(what, B, C, T, batch_stats)) return rc;
  const bool sums = grad_weight || grad_bias || (batch_stats && grad_x);
  if (sums)
    if (const int rc = check_bn_workspace(what, B, C, T, workspace, workspace_bytes)) return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const BatchNormArgs a = make_args(B, C, T);
  const dim3 grid(unsigned(wekws::batchnorm_tiles(B, C, T))), block(wekws::kBnThreads);
  const bool relu_b = relu != 0;
  float* coef = nullptr;
  if (sums) {
    coef = batch_stats && grad_x ? ws_coef(workspace, B, C, T) : nullptr;
    double* partial = ws_partial(workspace);
    const bool vec = T % 4 == 0 && aligned16(x) && aligned16(grad_y) && (!relu_b || aligned16(y));
    if (vec && relu_b) hipLaunchKernelGGL((wekws::batchnorm_grad_sums_kernel<4, true>), grid, block, 0, s, x, y, grad_y, save_mean, partial, a);
    else if (vec) hipLaunchKernelGGL((wekws::batchnorm_grad_sums_kernel<4, false>), grid, block, 0, s, x, y, grad_y, save_mean, partial, a);
    else if (relu_b) hipLaunchKernelGGL((wekws::batchnorm_grad_sums_kernel<1, true>), grid, block, 0, s, x, y, grad_y, save_mean, partial, a);
    else hipLaunchKernelGGL((wekws::batchnorm_grad_sums_kernel<1, false>), grid, block, 0, s, x, y, grad_y, save_mean, partial, a);
    if (hipGetLastError() != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "%s: launch failed", what);
    hipLaunchKernelGGL(wekws::batchnorm_grad_fold_kernel, dim3(unsigned((C + wekws::kBnFoldChans - 1) / wekws::kBnFoldChans)), block, 0, s,
                       static_cast<const double*>(partial), wekws::batchnorm_partials(B, T), C, double(int64_t(B) * T), save_invstd, grad_weight,
                       grad_bias, coef);
    if (hipGetLastError() != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "%s: launch failed", what);
  }
  if (grad_x || grad_residual) {
    const bool batch = batch_stats != 0;
    const bool vec = T % 4 == 0 && aligned16(grad_y) && (!relu_b || aligned16(y)) && (!(batch && grad_x) || aligned16(x)) &&
                     aligned16(grad_x) && aligned16(grad_residual);
    if (vec && relu_b) launch_grad_x<4, true>(batch, grid, s, x, y, grad_y, weight, save_mean, save_invstd, coef, grad_x, grad_residual, a);
    else if (vec) launch_grad_x<4, false>(batch, grid, s, x, y, grad_y, weight, save_mean, save_invstd, coef, grad_x, grad_residual, a);
    else if (relu_b) launch_grad_x<1, true>(batch, grid, s, x, y, grad_y, weight, save_mean, save_invstd, coef, grad_x, grad_residual, a);
    else launch_grad_x<1, false>(batch, grid, s, x, y, grad_y, weight, save_mean, save_invstd, coef, grad_x, grad_residual, a);
    if (hipGetLastError() != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "%s: launch failed", what);
  }
  return WEKWS_HIP_OK;
}

}  // extern "C"
