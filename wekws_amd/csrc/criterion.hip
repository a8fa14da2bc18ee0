// The validation criterion: launches and C entry points (kernels: criterion.hip.h).
#include "criterion.hip.h"

namespace wekws {

static int crit_launched() { return hipGetLastError() == hipSuccess ? 0 : -3; }

int launch_criterion_max_pooling(const float* scores, int B, int T, int K, const int32_t* target, const int32_t* lengths,
                                 int min_duration, float* pooled, float* terms, int32_t* correct, float* loss,
                                 int32_t* num_correct, hipStream_t stream) {
  hipLaunchKernelGGL(criterion_max_pooling_kernel, dim3(unsigned((B + 3) / 4)), dim3(256), 0, stream, scores, B, T, K, target,
                     lengths, min_duration, pooled, terms, correct);
  hipLaunchKernelGGL(criterion_sum_kernel, dim3(1), dim3(256), 0, stream, terms, int64_t(B) * K, float(B), loss, correct,
                     static_cast<const int32_t*>(nullptr), B, 1, num_correct);
  return crit_launched();
}

int launch_criterion_ce(const float* logits, int B, int D, const int32_t* target, float* loss_rows, int32_t* pred,
                        int32_t* correct, float* loss, int32_t* num_correct, hipStream_t stream) {
  hipLaunchKernelGGL(criterion_ce_kernel, dim3(unsigned((B + 3) / 4)), dim3(256), 0, stream, logits, B, D, target, loss_rows,
                     pred, correct);
  hipLaunchKernelGGL(criterion_sum_kernel, dim3(1), dim3(256), 0, stream, loss_rows, int64_t(B), float(B), loss, correct,
                     static_cast<const int32_t*>(nullptr), B, 1, num_correct);
  return crit_launched();
}

int launch_ctc_loss(const float* logits, int B, int T, int V, const int32_t* targets, int Lmax, const int32_t* logit_lengths,
                    const int32_t* target_lengths, float* loss_rows, float* loss, float* probs, float* lp, float* stats,
                    hipStream_t stream) {
  const int64_t frames = int64_t(B) * T;
  hipLaunchKernelGGL(ctc_loss_lp_kernel, dim3(unsigned((frames + 3) / 4)), dim3(256), 0, stream, logits, B, T, V, targets, Lmax,
                     logit_lengths, target_lengths, lp, probs, stats);
  const int W = 2 * Lmax + 1;
  const int threads = W <= 64 ? 64 : 256;                    // one wave needs no cross-wave barrier
  const size_t lds = (size_t(2) * W + size_t(Lmax > 0 ? Lmax : 1)) * 4;
  hipLaunchKernelGGL(ctc_loss_alpha_kernel, dim3(B), dim3(threads), lds, stream, lp, T, V, targets, Lmax, logit_lengths,
                     target_lengths, loss_rows);
  hipLaunchKernelGGL(criterion_sum_kernel, dim3(1), dim3(256), 0, stream, loss_rows, int64_t(B), float(B), loss,
                     static_cast<const int32_t*>(nullptr), static_cast<const int32_t*>(nullptr), 0, 0,
                     static_cast<int32_t*>(nullptr));
  return crit_launched();
}

int launch_ctc_edit_distance(const char* beams, size_t beam_stride, int PB, int cap, int B, const int32_t* targets, int Lmax,
                             const int32_t* target_lengths, int32_t* dist, int32_t* totals, hipStream_t stream) {
  hipLaunchKernelGGL(ctc_edit_distance_kernel, dim3(B), dim3(64), size_t(3) * (Lmax + 1) * 4, stream, beams, beam_stride, PB,
                     cap, targets, Lmax, target_lengths, dist);
  if (totals)
    hipLaunchKernelGGL(criterion_sum_kernel, dim3(1), dim3(256), 0, stream, static_cast<const float*>(nullptr), int64_t(0), 1.0f,
                       static_cast<float*>(nullptr), target_lengths, static_cast<const int32_t*>(dist), B, Lmax, totals);
  return crit_launched();
}

}  // namespace wekws

// ------------------------------------------------------------------------------------------------ C ABI
#include "host_util.h"

namespace {

int launch_fail(const char* what) {
  return fail(WEKWS_HIP_EDEVICE, "%s launch failed: %s", what, hipGetErrorString(hipGetLastError()));
}

}  // namespace

extern "C" {

int wekws_hip_criterion_max_pooling(const float* scores, int B, int T, int K, const int32_t* target, const int32_t* lengths,
                                    int min_duration, float* pooled, float* loss_terms, int32_t* correct, float* loss,
                                    int32_t* num_correct, void* stream) {
  if (!scores || !target || !pooled || !loss_terms || !correct || !loss || !num_correct)
    return fail(WEKWS_HIP_EINVAL, "criterion_max_pooling: NULL argument");
  if (B <= 0 || T <= 0 || K <= 0) return fail(WEKWS_HIP_EINVAL, "criterion_max_pooling: B=%d T=%d K=%d (all must be >= 1)", B, T, K);
  if (wekws::launch_criterion_max_pooling(scores, B, T, K, target, lengths, min_duration, pooled, loss_terms, correct, loss,
                                          num_correct, static_cast<hipStream_t>(stream)))
    return launch_fail("criterion_max_pooling");
  return WEKWS_HIP_OK;
}

int wekws_hip_criterion_ce(const float* logits, int B, int D, const int32_t* target, float* loss_rows, int32_t* pred,
                           int32_t* correct, float* loss, int32_t* num_correct, void* stream) {
  if (!logits || !target || !loss_rows || !pred || !correct || !loss || !num_correct)
    return fail(WEKWS_HIP_EINVAL, "criterion_ce: NULL argument");
  if (B <= 0 || D <= 0) return fail(WEKWS_HIP_EINVAL, "criterion_ce: B=%d D=%d (both must be >= 1)", B, D);
  if (wekws::launch_criterion_ce(logits, B, D, target, loss_rows, pred, correct, loss, num_correct,
                                 static_cast<hipStream_t>(stream)))
    return launch_fail("criterion_ce");
  return WEKWS_HIP_OK;
}

size_t wekws_hip_ctc_loss_workspace_bytes(int B, int T, int Lmax) {
  if (B <= 0 || T <= 0 || Lmax < 0) return 0;
  return size_t(B) * size_t(T) * (size_t(Lmax) + 1) * sizeof(float);
}

int wekws_hip_ctc_loss(const float* logits, int B, int T, int V, const int32_t* targets, int Lmax, const int32_t* logit_lengths,
                       const int32_t* target_lengths, float* loss_rows, float* loss, float* probs, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (!logits || !logit_lengths || !target_lengths || !loss_rows || !loss || !workspace || (Lmax > 0 && !targets))
    return fail(WEKWS_HIP_EINVAL, "ctc_loss: NULL argument");
  if (B <= 0 || T <= 0 || V <= 0 || Lmax < 0 || Lmax > wekws::kCtcLossMaxLabels)
    return fail(WEKWS_HIP_EINVAL, "ctc_loss: B=%d T=%d V=%d Lmax=%d (B, T, V >= 1; 0 <= Lmax <= %d)", B, T, V, Lmax,
                wekws::kCtcLossMaxLabels);
  if ((int64_t(B) * T + 3) / 4 > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "ctc_loss: too many frames for one launch");
  const size_t need = wekws_hip_ctc_loss_workspace_bytes(B, T, Lmax);
  if (workspace_bytes < need)
    return fail(WEKWS_HIP_EINVAL, "ctc_loss: workspace of %zu bytes, need %zu (wekws_hip_ctc_loss_workspace_bytes)", workspace_bytes, need);
  if (wekws::launch_ctc_loss(logits, B, T, V, targets, Lmax, logit_lengths, target_lengths, loss_rows, loss, probs,
                             static_cast<float*>(workspace), nullptr, static_cast<hipStream_t>(stream)))
    return launch_fail("ctc_loss");
  return WEKWS_HIP_OK;
}

int wekws_hip_ctc_edit_distance(const void* beams, int path_beam, int cap, int B, const int32_t* targets, int Lmax,
                                const int32_t* target_lengths, int32_t* dist, int32_t* totals, void* stream) {
  if (!beams || !target_lengths || !dist || (Lmax > 0 && !targets)) return fail(WEKWS_HIP_EINVAL, "ctc_edit_distance: NULL argument");
  if (B <= 0 || cap < 1 || path_beam < 1 || path_beam > wekws::kEditMaxPathBeam || Lmax < 0 || Lmax > wekws::kEditMaxLabels)
    return fail(WEKWS_HIP_EINVAL, "ctc_edit_distance: B=%d cap=%d path_beam=%d (1..%d) Lmax=%d (0..%d)", B, cap, path_beam,
                wekws::kEditMaxPathBeam, Lmax, wekws::kEditMaxLabels);
  if (wekws::launch_ctc_edit_distance(static_cast<const char*>(beams), wekws::edit_beam_bytes(path_beam, cap), path_beam, cap, B,
                                      targets, Lmax, target_lengths, dist, totals, static_cast<hipStream_t>(stream)))
    return launch_fail("ctc_edit_distance");
  return WEKWS_HIP_OK;
}

}  // extern "C"
