// The trainable GRU's recurrent scan: launches and C entry points (kernels: gru_train.hip.h; the plan: gru_train_plan.h).
#include "gru_train.hip.h"

#include "host_util.h"

namespace {

int check_shape(const char* what, int B, int T, int H) {
  if (const char* why = wekws::gru_scan_check(B, T, H)) return fail(WEKWS_HIP_EINVAL, "%s: %s (B=%d T=%d H=%d)", what, why, B, T, H);
  return WEKWS_HIP_OK;
}

template <int H>
bool launch_fwd(const float* gi, const float* w_hh, const float* b_hh, const float* h0, int B, int T, float* y, float* hn,
                float* reserve, hipStream_t s) {
  hipLaunchKernelGGL(wekws::gru_scan_fwd<H>, dim3(unsigned(wekws::gru_scan_grid(B))), dim3(wekws::kGruTrainThreads),
                     size_t(wekws::gru_scan_fwd_lds_bytes(H)), s, gi, w_hh, b_hh, h0, B, T, y, hn, reserve);
  return hipGetLastError() == hipSuccess;
}

template <int H>
bool launch_bwd(const float* grad_y, const float* grad_hn, const float* y, const float* h0, const float* reserve, const float* w_hh,
                int B, int T, float* grad_gi, float* grad_gh, float* grad_h0, hipStream_t s) {
  hipLaunchKernelGGL(wekws::gru_scan_bwd<H>, dim3(unsigned(wekws::gru_scan_grid(B))), dim3(wekws::kGruTrainThreads),
                     size_t(wekws::gru_scan_bwd_lds_bytes(H)), s, grad_y, grad_hn, y, h0, reserve, w_hh, B, T, grad_gi, grad_gh, grad_h0);
  return hipGetLastError() == hipSuccess;
}

// the built hidden sizes: a register array indexed at run time would go to scratch, so H is a template argument
#define GRU_TRAIN_FOR_H(CALL)                                                                                          \
  switch (H) {                                                                                                         \
    case 16: ok = CALL(16); break;                                                                                     \
    case 32: ok = CALL(32); break;                                                                                     \
    case 48: ok = CALL(48); break;                                                                                     \
    case 64: ok = CALL(64); break;                                                                                     \
    case 80: ok = CALL(80); break;                                                                                     \
    case 96: ok = CALL(96); break;                                                                                     \
    case 112: ok = CALL(112); break;                                                                                   \
    case 128: ok = CALL(128); break;                                                                                   \
    default: ok = false;                                                                                               \
  }

}  // namespace

extern "C" {

size_t wekws_hip_gru_scan_reserve_bytes(int B, int T, int H) {
  if (wekws::gru_scan_check(B, T, H)) {
    fail(WEKWS_HIP_EINVAL, "gru_scan_reserve_bytes: B=%d T=%d H=%d", B, T, H);
    return 0;
  }
  return size_t(wekws::gru_scan_reserve_bytes(B, T, H));
}

int wekws_hip_gru_scan_forward(const float* gi, const float* w_hh, const float* b_hh, const float* h0, int B, int T, int H, float* y,
                               float* hn, float* reserve, void* stream) {
  if (!gi || !w_hh || !y || !hn) return fail(WEKWS_HIP_EINVAL, "gru_scan_forward: NULL argument (gi, w_hh, y and hn are needed)");
  if (const int rc = check_shape("gru_scan_forward", B, T, H)) return rc;
  if (!aligned16(gi) || !aligned16(b_hh) || !aligned16(h0) || !aligned16(y) || !aligned16(hn) || !aligned16(reserve))
    return fail(WEKWS_HIP_EINVAL, "gru_scan_forward: every tensor must be 16-byte aligned");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  bool ok;
#define CALL(HH) launch_fwd<HH>(gi, w_hh, b_hh, h0, B, T, y, hn, reserve, s)
  GRU_TRAIN_FOR_H(CALL)
#undef CALL
  if (!ok) return fail(WEKWS_HIP_EDEVICE, "gru_scan_forward launch failed");
  return WEKWS_HIP_OK;
}

int wekws_hip_gru_scan_backward(const float* grad_y, const float* grad_hn, const float* y, const float* h0, const float* reserve,
                                const float* w_hh, int B, int T, int H, float* grad_gi, float* grad_gh, float* grad_h0, void* stream) {
  if (!y || !reserve || !w_hh || !grad_gi || !grad_gh)
    return fail(WEKWS_HIP_EINVAL, "gru_scan_backward: NULL argument (y, reserve, w_hh, grad_gi and grad_gh are needed)");
  if (const int rc = check_shape("gru_scan_backward", B, T, H)) return rc;
  if (!aligned16(grad_y) || !aligned16(grad_hn) || !aligned16(y) || !aligned16(h0) || !aligned16(reserve) || !aligned16(grad_gi) ||
      !aligned16(grad_gh) || !aligned16(grad_h0))
    return fail(WEKWS_HIP_EINVAL, "gru_scan_backward: every tensor must be 16-byte aligned");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  bool ok;
#define CALL(HH) launch_bwd<HH>(grad_y, grad_hn, y, h0, reserve, w_hh, B, T, grad_gi, grad_gh, grad_h0, s)
  GRU_TRAIN_FOR_H(CALL)
#undef CALL
  if (!ok) return fail(WEKWS_HIP_EDEVICE, "gru_scan_backward launch failed");
  return WEKWS_HIP_OK;
}

}  // extern "C"
