// Handle, launchers and C ABI of the global CMVN statistics (cmvn_stats.hip.h, cmvn_stats_plan.h).
#include "cmvn_stats.hip.h"

#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "host_util.h"

struct wekws_hip_cmvn_stats {
  int device = 0, dim = 0;
  char* d_acc = nullptr;                            // (2, dim) doubles, then {frames, bad rows} int64: the running totals
  void* scratch = nullptr;                          // the tiles' partials of the call under way
  size_t scratch_bytes = 0;
  std::mutex mu;
  size_t acc_bytes() const { return (size_t(2) * dim + 2) * sizeof(double); }
  double* acc() const { return reinterpret_cast<double*>(d_acc); }
  int64_t* counts() const { return reinterpret_cast<int64_t*>(d_acc + size_t(2) * dim * sizeof(double)); }
};

extern "C" {

int wekws_hip_cmvn_stats_plan(int B, int T, int D, int64_t out[3]) {
  if (!out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (wekws::cmvn_stats_check(B, T, D)) return fail(WEKWS_HIP_EINVAL, "cmvn_stats_plan: B=%d T=%d D=%d", B, T, D);
  out[0] = wekws::cmvn_tile_frames(D);
  out[1] = wekws::cmvn_tiles(B, T, D);
  out[2] = wekws::cmvn_scratch_bytes(B, T, D);
  return WEKWS_HIP_OK;
}

void wekws_hip_cmvn_stats_destroy(void* h) {
  wekws_hip_cmvn_stats* o = static_cast<wekws_hip_cmvn_stats*>(h);
  if (!o) return;
  DeviceGuard g(o->device);
  (void)hipDeviceSynchronize();
  if (o->d_acc) (void)hipFree(o->d_acc);
  if (o->scratch) (void)hipFree(o->scratch);
  delete o;
}

int wekws_hip_cmvn_stats_create(int dim, int device, void** out) {
  if (!out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  if (dim < 1 || dim > wekws::kCmvnMaxDim) return fail(WEKWS_HIP_EINVAL, "cmvn_stats_create: dim %d outside 1..%d", dim, wekws::kCmvnMaxDim);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(WEKWS_HIP_EDEVICE, "device %d of %d", device, ndev);
  wekws_hip_cmvn_stats* o = new (std::nothrow) wekws_hip_cmvn_stats;
  if (!o) return fail(WEKWS_HIP_ENOMEM, "host allocation failed");
  o->device = device;
  o->dim = dim;
  DeviceGuard g(device);
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&o->d_acc), o->acc_bytes());
  if (e == hipSuccess) e = hipMemset(o->d_acc, 0, o->acc_bytes());
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = hip_fail(e, "cmvn_stats create");
    wekws_hip_cmvn_stats_destroy(o);
    return rc;
  }
  *out = o;
  return WEKWS_HIP_OK;
}

int wekws_hip_cmvn_stats_update(void* h, const float* feats, int B, int T, const int32_t* lengths, void* stream_) {
  wekws_hip_cmvn_stats* o = static_cast<wekws_hip_cmvn_stats*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (wekws::cmvn_stats_check(B, T, o->dim)) return fail(WEKWS_HIP_EINVAL, "cmvn_stats_update: B=%d T=%d (at most 2^31 - 1 frames a call)", B, T);
  if (B == 0 || T == 0) return WEKWS_HIP_OK;
  if (!feats) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(o->mu);
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream_);
  const int D = o->dim;
  const size_t need = size_t(wekws::cmvn_scratch_bytes(B, T, D));
  if (need > o->scratch_bytes) {
    if (stream_is_capturing(s)) return fail(WEKWS_HIP_EINVAL, "cmvn_stats_update: %zu bytes of partials need a larger scratch: not inside a capture", need);
    if (o->scratch) (void)hipFree(o->scratch);      // (synchronises: no launch still uses it)
    o->scratch = nullptr; o->scratch_bytes = 0;
    HIP_TRY(hipMalloc(&o->scratch, need));
    o->scratch_bytes = need;
  }
  const int64_t tiles = wekws::cmvn_tiles(B, T, D);
  double* const partial = static_cast<double*>(o->scratch);
  const wekws::CmvnDiv by_T = wekws::cmvn_div(T);
  hipLaunchKernelGGL(wekws::cmvn_stats_tile_kernel, dim3(unsigned(tiles)), dim3(wekws::kCmvnThreads), 0, s, feats, T, D, lengths, B * T,
                     int(wekws::cmvn_tile_frames(D)), wekws::cmvn_lane_bins(D), wekws::cmvn_lane_frames(D), by_T.mul, by_T.shift, partial);
  hipError_t e = hipGetLastError();
  const unsigned groups = unsigned((D + wekws::kCmvnFoldCols - 1) / wekws::kCmvnFoldCols);
  const int64_t segs = wekws::cmvn_fold_segments(tiles);
  double* const seg_sums = partial + tiles * 2 * D;
  if (e == hipSuccess && segs) {
    hipLaunchKernelGGL(wekws::cmvn_stats_fold_kernel, dim3(unsigned(segs), groups), dim3(wekws::kCmvnThreads), 0, s, partial, int(tiles),
                       wekws::kCmvnFoldSeg, D, seg_sums, static_cast<const int32_t*>(nullptr), 0, 0, static_cast<int64_t*>(nullptr));
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    const int rows = int(segs ? segs : tiles);
    hipLaunchKernelGGL(wekws::cmvn_stats_fold_kernel, dim3(1, groups + 1), dim3(wekws::kCmvnThreads), 0, s, segs ? seg_sums : partial, rows, rows, D,
                       o->acc(), lengths, B, T, o->counts());
    e = hipGetLastError();
  }
  if (e != hipSuccess) return hip_fail(e, "cmvn_stats_update launch");
  return WEKWS_HIP_OK;
}

int wekws_hip_cmvn_stats_reset(void* h, void* stream_) {
  wekws_hip_cmvn_stats* o = static_cast<wekws_hip_cmvn_stats*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  std::lock_guard<std::mutex> lk(o->mu);
  DeviceGuard g(o->device);
  HIP_TRY(hipMemsetAsync(o->d_acc, 0, o->acc_bytes(), static_cast<hipStream_t>(stream_)));
  return WEKWS_HIP_OK;
}

int wekws_hip_cmvn_stats_read(void* h, double* mean_stat, double* var_stat, int64_t counts[2], void* stream_) {
  wekws_hip_cmvn_stats* o = static_cast<wekws_hip_cmvn_stats*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (!mean_stat || !var_stat || !counts) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(o->mu);
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream_);
  if (stream_is_capturing(s)) return fail(WEKWS_HIP_EINVAL, "cmvn_stats_read synchronises: not inside a capture");
  std::vector<double> host(size_t(2) * o->dim + 2);
  HIP_TRY(hipMemcpyAsync(host.data(), o->d_acc, o->acc_bytes(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  std::memcpy(mean_stat, host.data(), size_t(o->dim) * sizeof(double));
  std::memcpy(var_stat, host.data() + o->dim, size_t(o->dim) * sizeof(double));
  std::memcpy(counts, host.data() + size_t(2) * o->dim, 2 * sizeof(int64_t));
  return WEKWS_HIP_OK;
}

}  // extern "C"
