// The criterion's backward pass: launches and C entry points (kernels: criterion_grad.hip.h).
#include "criterion_grad.hip.h"

namespace wekws {

static int crit_grad_launched() { return hipGetLastError() == hipSuccess ? 0 : -3; }

int launch_criterion_max_pooling_grad(const float* scores, int B, int T, int K, const int32_t* target, const int32_t* lengths,
                                      int min_duration, const float* upstream, int divisor, float* grad, hipStream_t stream) {
  const int64_t waves = int64_t(B) * K;
  hipLaunchKernelGGL(criterion_max_pooling_grad_kernel, dim3(unsigned((waves + 3) / 4)), dim3(256), 0, stream, scores, B, T, K,
                     target, lengths, min_duration, upstream, divisor, grad);
  return crit_grad_launched();
}

int launch_criterion_ce_grad(const float* logits, int B, int D, const int32_t* target, const float* upstream, int divisor,
                             float* grad, hipStream_t stream) {
  hipLaunchKernelGGL(criterion_ce_grad_kernel, dim3(unsigned((B + 3) / 4)), dim3(256), 0, stream, logits, B, D, target, upstream,
                     divisor, grad);
  return crit_grad_launched();
}

int launch_ctc_loss_grad(const float* logits, int B, int T, int V, const int32_t* targets, int Lmax, const int32_t* logit_lengths,
                         const int32_t* target_lengths, const float* upstream, int divisor, float* loss_rows, float* loss,
                         float* grad, char* workspace, hipStream_t stream) {
  const CtcGradWorkspace ws = ctc_grad_workspace(B, T, Lmax);
  float* lp = reinterpret_cast<float*>(workspace + ws.lp);
  float* stats = reinterpret_cast<float*>(workspace + ws.stats);
  double* ab = reinterpret_cast<double*>(workspace + ws.ab);
  double* pp = reinterpret_cast<double*>(workspace + ws.pp);
  double* nll = reinterpret_cast<double*>(workspace + ws.nll);
  int32_t* link = reinterpret_cast<int32_t*>(workspace + ws.link);
  // the forward's own three launches: loss_rows and loss come out of the same kernels with the same bits
  if (launch_ctc_loss(logits, B, T, V, targets, Lmax, logit_lengths, target_lengths, loss_rows, loss, nullptr, lp, stats, stream))
    return -3;
  const int W = 2 * Lmax + 1;
  const int threads = W <= 64 ? 64 : 256;
  const int lds_mode = W <= kCtcGradLdsStates ? 1 : 0;
  const size_t lds = (lds_mode ? size_t(2) * W * sizeof(double) : 0) + size_t(Lmax > 0 ? Lmax : 1) * sizeof(int32_t);
  hipLaunchKernelGGL(ctc_grad_alpha_beta_kernel, dim3(B), dim3(threads), lds, stream, lp, T, V, targets, Lmax, logit_lengths,
                     target_lengths, ab, pp, nll, link, lds_mode);
  hipLaunchKernelGGL(ctc_grad_kernel, dim3(unsigned(int64_t(B) * T)), dim3(256), 0, stream, logits, T, V, targets, Lmax,
                     logit_lengths, target_lengths, stats, ab, nll, link, upstream, divisor, grad);
  return crit_grad_launched();
}

}  // namespace wekws

// ------------------------------------------------------------------------------------------------ C ABI
#include "host_util.h"

namespace {

int grad_launch_fail(const char* what) {
  return fail(WEKWS_HIP_EDEVICE, "%s launch failed: %s", what, hipGetErrorString(hipGetLastError()));
}

}  // namespace

extern "C" {

int wekws_hip_criterion_max_pooling_grad(const float* scores, int B, int T, int K, const int32_t* target, const int32_t* lengths,
                                         int min_duration, const float* upstream, int divisor, float* grad, void* stream) {
  if (!scores || !target || !grad) return fail(WEKWS_HIP_EINVAL, "criterion_max_pooling_grad: NULL argument");
  if (B <= 0 || T <= 0 || K <= 0)
    return fail(WEKWS_HIP_EINVAL, "criterion_max_pooling_grad: B=%d T=%d K=%d (all must be >= 1)", B, T, K);
  if (divisor < 1) return fail(WEKWS_HIP_EINVAL, "criterion_max_pooling_grad: divisor=%d (must be >= 1)", divisor);
  if ((int64_t(B) * K + 3) / 4 > 0x7fffffffLL)
    return fail(WEKWS_HIP_EINVAL, "criterion_max_pooling_grad: too many (utterance, keyword) pairs for one launch");
  if (wekws::launch_criterion_max_pooling_grad(scores, B, T, K, target, lengths, min_duration, upstream, divisor, grad,
                                               static_cast<hipStream_t>(stream)))
    return grad_launch_fail("criterion_max_pooling_grad");
  return WEKWS_HIP_OK;
}

int wekws_hip_criterion_ce_grad(const float* logits, int B, int D, const int32_t* target, const float* upstream, int divisor,
                                float* grad, void* stream) {
  if (!logits || !target || !grad) return fail(WEKWS_HIP_EINVAL, "criterion_ce_grad: NULL argument");
  if (B <= 0 || D <= 0) return fail(WEKWS_HIP_EINVAL, "criterion_ce_grad: B=%d D=%d (both must be >= 1)", B, D);
  if (divisor < 1) return fail(WEKWS_HIP_EINVAL, "criterion_ce_grad: divisor=%d (must be >= 1)", divisor);
  if (wekws::launch_criterion_ce_grad(logits, B, D, target, upstream, divisor, grad, static_cast<hipStream_t>(stream)))
    return grad_launch_fail("criterion_ce_grad");
  return WEKWS_HIP_OK;
}

size_t wekws_hip_ctc_loss_grad_workspace_bytes(int B, int T, int Lmax) {
  if (B <= 0 || T <= 0 || Lmax < 0) return 0;
  return wekws::ctc_grad_workspace(B, T, Lmax).total;
}

int wekws_hip_ctc_loss_grad(const float* logits, int B, int T, int V, const int32_t* targets, int Lmax,
                            const int32_t* logit_lengths, const int32_t* target_lengths, const float* upstream, int divisor,
                            float* loss_rows, float* loss, float* grad, void* workspace, size_t workspace_bytes, void* stream) {
  if (!logits || !logit_lengths || !target_lengths || !loss_rows || !loss || !grad || !workspace || (Lmax > 0 && !targets))
    return fail(WEKWS_HIP_EINVAL, "ctc_loss_grad: NULL argument");
  if (B <= 0 || T <= 0 || V <= 0 || Lmax < 0 || Lmax > wekws::kCtcLossMaxLabels)
    return fail(WEKWS_HIP_EINVAL, "ctc_loss_grad: B=%d T=%d V=%d Lmax=%d (B, T, V >= 1; 0 <= Lmax <= %d)", B, T, V, Lmax,
                wekws::kCtcLossMaxLabels);
  if (divisor < 1) return fail(WEKWS_HIP_EINVAL, "ctc_loss_grad: divisor=%d (must be >= 1)", divisor);
  if (int64_t(B) * T > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "ctc_loss_grad: too many frames for one launch");
  const size_t need = wekws_hip_ctc_loss_grad_workspace_bytes(B, T, Lmax);
  if (workspace_bytes < need)
    return fail(WEKWS_HIP_EINVAL, "ctc_loss_grad: workspace of %zu bytes, need %zu (wekws_hip_ctc_loss_grad_workspace_bytes)",
                workspace_bytes, need);
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(WEKWS_HIP_EINVAL, "ctc_loss_grad: workspace must be 8-byte aligned");
  if (wekws::launch_ctc_loss_grad(logits, B, T, V, targets, Lmax, logit_lengths, target_lengths, upstream, divisor, loss_rows, loss,
                                  grad, static_cast<char*>(workspace), static_cast<hipStream_t>(stream)))
    return grad_launch_fail("ctc_loss_grad");
  return WEKWS_HIP_OK;
}

}  // extern "C"
