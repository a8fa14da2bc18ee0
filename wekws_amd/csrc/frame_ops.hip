// Context expansion + frame skip, the MFCC tail, the CTC first beam prune and DET scoring: the kernels of splice.hip.h, mfcc.hip.h,
// topk.hip.h and det.hip.h (emitted here and nowhere else) and their C entry points.
#include "host_util.h"
#include "mfcc.hip.h"
#include "splice.hip.h"
#include "topk.hip.h"
#include "det.hip.h"

namespace wekws {
// for the streaming front end in MFCC mode (declared in stream_frontend.hip.h): the kernels of mfcc.hip.h live in this unit
WEKWS_LOCAL int build_dct_lifter_matrix(float* D, int num_bins, int num_ceps, float lifter, hipStream_t stream) {
  return launch_dct_lifter_matrix(D, num_bins, num_ceps, lifter, stream);
}
}  // namespace wekws

extern "C" {

// --------------------------------------------- context expansion + frame skip ---------------------------------------------
int wekws_hip_splice_frames(int T, int right, int skip) {
  if (skip <= 0 || right < 0 || T <= 0) return 0;
  // init_dataset.py:50  feats_ctx[:, :T - right]  -- a NEGATIVE bound (an utterance shorter than its right context) is Python's
  // "all but the last right - T": 2 T - right frames survive -- then :64-65 keeps every skip-th
  const int kept = T >= right ? T - right : (2 * T > right ? 2 * T - right : 0);
  return (kept + skip - 1) / skip;
}

int wekws_hip_splice(const float* feats, int B, int T, int F, int left, int right, int skip, float* out, void* stream_) {
  if (!feats || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (B < 0 || T < 0 || F <= 0 || left < 0 || right < 0 || skip <= 0)
    return fail(WEKWS_HIP_EINVAL, "B=%d T=%d F=%d left=%d right=%d skip=%d", B, T, F, left, right, skip);
  // init_dataset.py:45-48: the left-margin loop reads feats_ctx[:, left] -- the reference raises IndexError for left >= T (any B)
  if (left >= 1 && left >= T)
    return fail(WEKWS_HIP_EINVAL, "splice: left context %d >= T = %d (the reference's left-margin loop raises IndexError)", left, T);
  const int To = wekws_hip_splice_frames(T, right, skip);
  if (B == 0 || To == 0) return WEKWS_HIP_OK;
  if ((int64_t(B) * To * (left + right + 1) * F + 255) / 256 > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "splice: too many elements for one launch");
  const int rc = wekws::launch_splice(feats, B, T, F, left, right, skip, To, out, static_cast<hipStream_t>(stream_));
  if (rc) return fail(rc, "splice launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}

// --------------------------------------------- MFCC tail (DCT + lifter) ---------------------------------------------
int wekws_hip_dct_lifter(const float* logmel, int64_t rows, int num_bins, int num_ceps, float cepstral_lifter, float* out,
                         void* stream_) {
  if (!logmel || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (rows < 0 || num_bins <= 0 || num_bins > wekws::kMfccMaxBins || num_ceps <= 0 || num_ceps > num_bins || cepstral_lifter < 0.f)
    return fail(WEKWS_HIP_EINVAL, "rows=%lld num_bins=%d num_ceps=%d lifter=%g (need 0 < num_ceps <= num_bins <= %d)",
                (long long)rows, num_bins, num_ceps, double(cepstral_lifter), wekws::kMfccMaxBins);
  if (rows == 0) return WEKWS_HIP_OK;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return fail(WEKWS_HIP_EDEVICE, "no HIP device");
  const int rc = wekws::launch_dct_lifter(logmel, rows, num_bins, num_ceps, cepstral_lifter, out, cus, static_cast<hipStream_t>(stream_));
  if (rc) return fail(rc, "dct_lifter launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}

// --------------------------------------------- CTC first beam prune ---------------------------------------------
int wekws_hip_softmax_topk(const float* logits, int64_t rows, int K, int k, float* probs, int32_t* idx, void* stream_) {
  if (!logits || !probs || !idx) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (rows < 0 || K <= 0 || k < 1 || k > wekws::kTopkMax) return fail(WEKWS_HIP_EINVAL, "rows=%lld K=%d k=%d (k must be 1..%d)", (long long)rows, K, k, wekws::kTopkMax);
  if (rows == 0) return WEKWS_HIP_OK;
  if ((rows + 3) / 4 > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "softmax_topk: too many rows for one launch");
  const int rc = wekws::launch_softmax_topk(logits, rows, K, k, probs, idx, static_cast<hipStream_t>(stream_));
  if (rc) return fail(rc, "softmax_topk launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}

// --------------------------------------------- DET scoring ---------------------------------------------
int wekws_hip_score_maxpool(const float* scores, int B, int T, int K, const int32_t* lengths, float* max_out,
                            int32_t* argmax_out, void* stream_) {
  if (!scores || !max_out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (B < 0 || T <= 0 || K <= 0) return fail(WEKWS_HIP_EINVAL, "B=%d T=%d K=%d", B, T, K);
  if (B == 0) return WEKWS_HIP_OK;
  if ((int64_t(B) * K + 3) / 4 > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "score_maxpool: too many rows for one launch");
  const int rc = wekws::launch_det_maxpool(scores, B, T, K, lengths, max_out, argmax_out, static_cast<hipStream_t>(stream_));
  if (rc) return fail(rc, "det_maxpool launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}

static int det_false_alarms(bool text6, const float* scores, int B, int T, int K, int keyword, const int32_t* lengths,
                            const double* thresholds, int n_thr, int window_shift, int32_t* alarms, void* stream_) {
  if (!scores || !thresholds || !alarms) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (B < 0 || T <= 0 || K <= 0 || keyword < 0 || keyword >= K || n_thr <= 0 || window_shift <= 0)
    return fail(WEKWS_HIP_EINVAL, "B=%d T=%d K=%d keyword=%d n_thr=%d window_shift=%d", B, T, K, keyword, n_thr, window_shift);
  if (B == 0) return WEKWS_HIP_OK;
  if ((int64_t(B) * n_thr + 255) / 256 > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "det_false_alarms: too many items for one launch");
  const int rc = wekws::launch_det_alarms(text6, scores, B, T, K, keyword, lengths, thresholds, n_thr, window_shift, alarms,
                                          static_cast<hipStream_t>(stream_));
  if (rc) return fail(rc, "det_alarm launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}
int wekws_hip_det_false_alarms(const float* scores, int B, int T, int K, int keyword, const int32_t* lengths,
                               const double* thresholds, int n_thr, int window_shift, int32_t* alarms, void* stream_) {
  return det_false_alarms(false, scores, B, T, K, keyword, lengths, thresholds, n_thr, window_shift, alarms, stream_);
}
int wekws_hip_det_false_alarms_text(const float* scores, int B, int T, int K, int keyword, const int32_t* lengths,
                                    const double* thresholds, int n_thr, int window_shift, int32_t* alarms, void* stream_) {
  return det_false_alarms(true, scores, B, T, K, keyword, lengths, thresholds, n_thr, window_shift, alarms, stream_);
}

}  // extern "C"
