// The optimiser step: launches and C entry points (kernels: optim.hip.h; the cut and the state block: optim_plan.h).
#include "optim.hip.h"

#include <cmath>

#include "host_util.h"

namespace {

using wekws::OptimState;

// [a, a + bytes) and [b, b + bytes) share a byte
bool overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y ? y - x < bytes : x - y < bytes;
}

// the tiles' sums of squares, folded down to at most kOptimFoldSeg doubles; -> where those lie and how many
int launch_sumsq(const float* grads, int64_t n, double* ws, hipStream_t s, const double** rows, int* nrows) {
  const int64_t tiles = wekws::optim_tiles(n), segs = wekws::optim_fold_segments(tiles);
  hipLaunchKernelGGL(wekws::grad_sumsq_kernel, dim3(unsigned(tiles)), dim3(wekws::kOptimThreads), 0, s, grads, n, ws);
  if (hipGetLastError() != hipSuccess) return 1;
  *rows = ws;
  *nrows = int(tiles);
  if (segs) {
    hipLaunchKernelGGL(wekws::clip_fold_kernel, dim3(unsigned(segs)), dim3(wekws::kOptimThreads), 0, s, ws, int(tiles), ws + tiles,
                       static_cast<float*>(nullptr), static_cast<OptimState*>(nullptr), 0.0, 0.0, 0.0, 0.0, 0);
    if (hipGetLastError() != hipSuccess) return 1;
    *rows = ws + tiles;
    *nrows = int(segs);
  }
  return 0;
}

int check_grads(const char* what, const float* grads, int64_t n, const void* workspace, size_t workspace_bytes) {
  if (wekws::optim_check(n)) return fail(WEKWS_HIP_EINVAL, "%s: n=%lld (1 .. %lld)", what, (long long)n, (long long)wekws::kOptimMaxElems);
  if (!aligned16(grads) || !aligned16(workspace)) return fail(WEKWS_HIP_EINVAL, "%s: every pointer must be 16-byte aligned", what);
  const size_t need = size_t(wekws::optim_workspace_bytes(n));
  if (workspace_bytes < need)
    return fail(WEKWS_HIP_EINVAL, "%s: workspace of %zu bytes, need %zu (wekws_hip_optim_plan)", what, workspace_bytes, need);
  return WEKWS_HIP_OK;
}

}  // namespace

extern "C" {

int wekws_hip_optim_plan(int64_t n, int64_t out[3]) {
  if (!out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (wekws::optim_check(n)) return fail(WEKWS_HIP_EINVAL, "optim_plan: n=%lld (1 .. %lld)", (long long)n, (long long)wekws::kOptimMaxElems);
  out[0] = wekws::kOptimTileFloats;
  out[1] = wekws::optim_tiles(n);
  out[2] = wekws::optim_workspace_bytes(n);
  return WEKWS_HIP_OK;
}

size_t wekws_hip_optim_state_bytes(void) { return sizeof(OptimState); }

int wekws_hip_clip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, void* state, double lr,
                             double beta1, double beta2, double eps, double weight_decay, double max_norm, int skip_nonfinite,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !state || !workspace) return fail(WEKWS_HIP_EINVAL, "clip_adam_step: NULL argument");
  if (const int rc = check_grads("clip_adam_step", grads, n, workspace, workspace_bytes)) return rc;
  if (!aligned16(params) || !aligned16(exp_avg) || !aligned16(exp_avg_sq) || !aligned16(state))
    return fail(WEKWS_HIP_EINVAL, "clip_adam_step: every pointer must be 16-byte aligned");
  const size_t bytes = size_t(n) * sizeof(float);
  if (overlap(params, grads, bytes) || overlap(params, exp_avg, bytes) || overlap(params, exp_avg_sq, bytes) ||
      overlap(grads, exp_avg, bytes) || overlap(grads, exp_avg_sq, bytes) || overlap(exp_avg, exp_avg_sq, bytes))
    return fail(WEKWS_HIP_EINVAL, "clip_adam_step: the four buffers must not overlap");
  // (written so that a NaN fails every test)
  if (!(lr >= 0.0 && lr < HUGE_VAL)) return fail(WEKWS_HIP_EINVAL, "clip_adam_step: lr=%g (must be finite and >= 0)", lr);
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
    return fail(WEKWS_HIP_EINVAL, "clip_adam_step: betas=(%g, %g) (both in [0, 1))", beta1, beta2);
  if (!(eps >= 0.0 && eps < HUGE_VAL)) return fail(WEKWS_HIP_EINVAL, "clip_adam_step: eps=%g (must be finite and >= 0)", eps);
  if (!(weight_decay >= 0.0 && weight_decay < HUGE_VAL))
    return fail(WEKWS_HIP_EINVAL, "clip_adam_step: weight_decay=%g (must be finite and >= 0)", weight_decay);
  if (!(max_norm > 0.0)) return fail(WEKWS_HIP_EINVAL, "clip_adam_step: max_norm=%g (must be > 0; +Inf: no clipping)", max_norm);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const double* rows = nullptr;
  int nrows = 0;
  bool bad = launch_sumsq(grads, n, static_cast<double*>(workspace), s, &rows, &nrows) != 0;
  if (!bad) {
    hipLaunchKernelGGL(wekws::clip_fold_kernel, dim3(1), dim3(wekws::kOptimThreads), 0, s, rows, nrows, static_cast<double*>(nullptr),
                       static_cast<float*>(nullptr), static_cast<OptimState*>(state), lr, beta1, beta2, max_norm, skip_nonfinite ? 1 : 0);
    bad = hipGetLastError() != hipSuccess;
  }
  if (!bad) {
    // 1 - beta in double, then rounded: the scalars torch's Adam hands to lerp_ / addcmul_
    const wekws::OptimHyper h{float(beta1), float(1.0 - beta1), float(beta2), float(1.0 - beta2), float(eps), float(weight_decay)};
    const int64_t work = (n >> 2) + (n & 3);
    hipLaunchKernelGGL(wekws::adam_apply_kernel, dim3(unsigned((work + wekws::kOptimThreads - 1) / wekws::kOptimThreads)),
                       dim3(wekws::kOptimThreads), 0, s, params, grads, exp_avg, exp_avg_sq, n, static_cast<const OptimState*>(state), h);
    bad = hipGetLastError() != hipSuccess;
  }
  if (bad) return fail(WEKWS_HIP_EDEVICE, "clip_adam_step launch failed");
  return WEKWS_HIP_OK;
}

int wekws_hip_grad_norm(const float* grads, int64_t n, float* norm_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!grads || !norm_out || !workspace) return fail(WEKWS_HIP_EINVAL, "grad_norm: NULL argument");
  if (const int rc = check_grads("grad_norm", grads, n, workspace, workspace_bytes)) return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const double* rows = nullptr;
  int nrows = 0;
  bool bad = launch_sumsq(grads, n, static_cast<double*>(workspace), s, &rows, &nrows) != 0;
  if (!bad) {
    hipLaunchKernelGGL(wekws::clip_fold_kernel, dim3(1), dim3(wekws::kOptimThreads), 0, s, rows, nrows, static_cast<double*>(nullptr), norm_out,
                       static_cast<OptimState*>(nullptr), 0.0, 0.0, 0.0, 0.0, 0);
    bad = hipGetLastError() != hipSuccess;
  }
  if (bad) return fail(WEKWS_HIP_EDEVICE, "grad_norm launch failed");
  return WEKWS_HIP_OK;
}

}  // extern "C"
