// Launchers, handle and C ABI of the streaming threshold detector (threshold_kws.hip.h).
#include "threshold_kws.hip.h"

namespace wekws {

int launch_threshold_kws_step(const ThresholdParams& p, const float* probs, int B, int Tcap, int Dcap, const int32_t* ids,
                              const int32_t* frames, int32_t* hit_frames, float* hit_scores, float* best, int32_t* best_frame,
                              int32_t* status, hipStream_t stream) {
  const int64_t n = int64_t(B) * p.K;
  hipLaunchKernelGGL(threshold_kws_step_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, stream, p, probs, B, Tcap, Dcap, ids,
                     frames, hit_frames, hit_scores, best, best_frame, status);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_threshold_kws_reset(const ThresholdParams& p, const int32_t* ids, int n, hipStream_t stream) {
  const int64_t e = int64_t(n) * p.K;
  hipLaunchKernelGGL(threshold_kws_reset_kernel, dim3(unsigned((e + 255) / 256)), dim3(256), 0, stream, p, ids, n);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace wekws

// ------------------------------------------------------------------------------------------------ C ABI
#include <new>

#include "host_util.h"

namespace {

struct ThresholdKws {
  int device = 0;
  wekws::ThresholdParams p{};
  double* d_thr = nullptr;
  wekws::ThresholdSlot* slots = nullptr;
};

}  // namespace

extern "C" {

void wekws_hip_threshold_kws_destroy(void* h) {
  ThresholdKws* o = static_cast<ThresholdKws*>(h);
  if (!o) return;
  DeviceGuard g(o->device);
  (void)hipDeviceSynchronize();
  if (o->d_thr) (void)hipFree(o->d_thr);
  if (o->slots) (void)hipFree(o->slots);
  delete o;
}

int wekws_hip_threshold_kws_create(int num_keywords, const double* thresholds, int window_shift, int max_streams, int device,
                                   void** out) {
  if (!out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  if (!thresholds) return fail(WEKWS_HIP_EINVAL, "threshold_kws: NULL thresholds");
  if (num_keywords < 1 || window_shift < 1 || max_streams < 1 || int64_t(num_keywords) * max_streams > 0x7fffffffLL)
    return fail(WEKWS_HIP_EINVAL, "threshold_kws: num_keywords=%d window_shift=%d max_streams=%d (each >= 1)", num_keywords,
                window_shift, max_streams);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(WEKWS_HIP_EDEVICE, "device %d of %d", device, ndev);
  ThresholdKws* o = new (std::nothrow) ThresholdKws;
  if (!o) return fail(WEKWS_HIP_ENOMEM, "host allocation failed");
  o->device = device;
  DeviceGuard g(device);
  wekws::ThresholdParams& p = o->p;
  p.K = num_keywords; p.window_shift = window_shift; p.n_streams = max_streams;
  const size_t nslots = size_t(num_keywords) * max_streams;
  hipError_t e = hipMalloc(&o->d_thr, size_t(num_keywords) * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(o->d_thr, thresholds, size_t(num_keywords) * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&o->slots, nslots * sizeof(wekws::ThresholdSlot));
  p.thresholds = o->d_thr; p.slots = o->slots;
  if (e == hipSuccess && wekws::launch_threshold_kws_reset(p, nullptr, max_streams, nullptr)) e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = hip_fail(e, "threshold_kws create");
    wekws_hip_threshold_kws_destroy(o);
    return rc;
  }
  *out = o;
  return WEKWS_HIP_OK;
}

int wekws_hip_threshold_kws_max_hits(void* h, int Tcap) {
  ThresholdKws* o = static_cast<ThresholdKws*>(h);
  if (!o || Tcap <= 0) return 0;
  return int((int64_t(Tcap) + o->p.window_shift - 1) / o->p.window_shift);
}

int wekws_hip_threshold_kws_step(void* h, const float* probs, int B, int Tcap, const int32_t* stream_ids, const int32_t* frames,
                                 int32_t* hit_frames, float* hit_scores, float* best, int32_t* best_frame, int32_t* status,
                                 void* stream) {
  ThresholdKws* o = static_cast<ThresholdKws*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (B < 0 || Tcap < 0) return fail(WEKWS_HIP_EINVAL, "threshold_kws_step: B=%d Tcap=%d", B, Tcap);
  if (B == 0) return WEKWS_HIP_OK;
  const int Dcap = wekws_hip_threshold_kws_max_hits(h, Tcap);
  if (!stream_ids || !best || !best_frame || (Tcap > 0 && (!probs || !hit_frames || !hit_scores)))
    return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (int64_t(B) * o->p.K > 0x7fffffffLL || int64_t(B) * o->p.K * (Dcap > 0 ? Dcap : 1) > 0x7fffffffLL * 256)
    return fail(WEKWS_HIP_EINVAL, "threshold_kws_step: B %d x K %d is out of range", B, o->p.K);
  DeviceGuard g(o->device);
  if (wekws::launch_threshold_kws_step(o->p, probs, B, Tcap, Dcap, stream_ids, frames, hit_frames, hit_scores, best, best_frame,
                                       status, static_cast<hipStream_t>(stream)))
    return hip_fail(hipGetLastError(), "threshold_kws_step launch");
  return WEKWS_HIP_OK;
}

int wekws_hip_threshold_kws_reset(void* h, const int32_t* ids, int n, void* stream) {
  ThresholdKws* o = static_cast<ThresholdKws*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (n < 0 || (n > 0 && !ids)) return fail(WEKWS_HIP_EINVAL, "threshold_kws_reset: n=%d", n);
  if (n == 0) return WEKWS_HIP_OK;
  if (int64_t(n) * o->p.K > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "threshold_kws_reset: n=%d is out of range", n);
  DeviceGuard g(o->device);
  if (wekws::launch_threshold_kws_reset(o->p, ids, n, static_cast<hipStream_t>(stream)))
    return hip_fail(hipGetLastError(), "threshold_kws_reset launch");
  return WEKWS_HIP_OK;
}

int wekws_hip_threshold_kws_state(void* h, int id, int keyword, wekws_hip_threshold_kws_slot* out, void* stream) {
  ThresholdKws* o = static_cast<ThresholdKws*>(h);
  if (!o || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (id < 0 || id >= o->p.n_streams || keyword < 0 || keyword >= o->p.K)
    return fail(WEKWS_HIP_EINVAL, "threshold_kws_state: stream %d outside 0..%d or keyword %d outside 0..%d", id, o->p.n_streams - 1,
                keyword, o->p.K - 1);
  static_assert(sizeof(wekws_hip_threshold_kws_slot) == sizeof(wekws::ThresholdSlot), "the public record is the slot");
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemcpyAsync(out, o->slots + size_t(id) * o->p.K + keyword, sizeof(wekws::ThresholdSlot), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, "threshold_kws_state");
  return WEKWS_HIP_OK;
}

}  // extern "C"
