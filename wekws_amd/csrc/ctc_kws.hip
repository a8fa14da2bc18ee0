// Launchers of the on-device CTC prefix beam search and keyword detection (ctc_kws.hip.h).
#include "ctc_kws.hip.h"

namespace wekws {

int launch_ctc_kws(const CtcParams& p, int mode, const float* probs, int B, int T, const int32_t* ids, const int32_t* counts,
                   CtcResult* results, char* beams, size_t beam_stride, hipStream_t stream) {
  // two LDS footprints: the reference's defaults (3 / 20) and everything up to 8 / 64
  if (p.K <= 4 && p.PB <= 32)
    hipLaunchKernelGGL((ctc_kws_kernel<4, 32>), dim3(B), dim3(64), 0, stream, p, mode, probs, T, ids, counts, results, beams,
                       beam_stride);
  else
    hipLaunchKernelGGL((ctc_kws_kernel<kCtcMaxScoreBeam, kCtcMaxPathBeam>), dim3(B), dim3(64), 0, stream, p, mode, probs, T,
                       ids, counts, results, beams, beam_stride);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_ctc_kws_reset(const CtcParams& p, const int32_t* ids, int n, int all, hipStream_t stream) {
  hipLaunchKernelGGL(ctc_kws_reset_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, p, ids, n, all);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_ctc_kws_init(const CtcParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(ctc_kws_init_kernel, dim3((p.n_slots + 255) / 256), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_ctc_kws_read_beam(const CtcParams& p, int id, char* out, hipStream_t stream) {
  hipLaunchKernelGGL(ctc_kws_read_beam_kernel, dim3(1), dim3(64), 0, stream, p, id, out);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace wekws

// ------------------------------------------------------------------------------------------------ C ABI
#include <cstddef>
#include <mutex>
#include <new>
#include <vector>

#include "host_util.h"

namespace {

struct CtcKws {
  int device = 0;
  wekws::CtcParams p{};   // the streaming slots
  char* slots = nullptr;
  uint32_t* tokset = nullptr;
  int32_t* kw = nullptr;
  std::mutex mu;          // the offline workspace
  char* ws = nullptr;
  size_t ws_bytes = 0;
};

}  // namespace

extern "C" {

int wekws_hip_ctc_kws_create(const wekws_hip_ctc_kws_desc* d, void** out) {
  if (!d || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  if (d->vocab < 1 || d->score_beam < 1 || d->score_beam > wekws::kCtcMaxScoreBeam || d->path_beam < 1 ||
      d->path_beam > wekws::kCtcMaxPathBeam || d->num_keywords < 0 || d->downsampling < 1 || d->max_streams < 0 ||
      d->prefix_capacity < 1 || d->token_set_len < 0)
    return fail(WEKWS_HIP_EINVAL, "ctc_kws: vocab=%d score_beam=%d (1..%d) path_beam=%d (1..%d) num_keywords=%d downsampling=%d "
                "max_streams=%d prefix_capacity=%d token_set_len=%d", d->vocab, d->score_beam, wekws::kCtcMaxScoreBeam,
                d->path_beam, wekws::kCtcMaxPathBeam, d->num_keywords, d->downsampling, d->max_streams, d->prefix_capacity,
                d->token_set_len);
  if (d->num_keywords > 0 && (!d->keyword_tokens || !d->keyword_offsets))
    return fail(WEKWS_HIP_EINVAL, "ctc_kws: keywords given without tokens / offsets");
  std::vector<int32_t> kw(size_t(d->num_keywords) + 1, 0);
  if (d->num_keywords > 0) {
    if (d->keyword_offsets[0] != 0) return fail(WEKWS_HIP_EINVAL, "ctc_kws: keyword_offsets[0] must be 0");
    for (int k = 0; k < d->num_keywords; ++k) {
      if (d->keyword_offsets[k + 1] <= d->keyword_offsets[k])
        return fail(WEKWS_HIP_EINVAL, "ctc_kws: keyword %d is empty (offsets must increase)", k);
      kw[k + 1] = d->keyword_offsets[k + 1];
    }
    const int total = kw.back();
    for (int i = 0; i < total; ++i) {
      if (d->keyword_tokens[i] < 0 || d->keyword_tokens[i] >= d->vocab)
        return fail(WEKWS_HIP_EINVAL, "ctc_kws: keyword token %d outside the vocabulary (%d)", d->keyword_tokens[i], d->vocab);
      kw.push_back(d->keyword_tokens[i]);
    }
  }
  std::vector<uint32_t> set;
  if (d->token_set) {
    set.assign((size_t(d->vocab) + 31) / 32, 0u);
    for (int i = 0; i < d->token_set_len; ++i) {
      const int s = d->token_set[i];
      if (s < 0 || s >= d->vocab) return fail(WEKWS_HIP_EINVAL, "ctc_kws: token set entry %d outside the vocabulary", s);
      set[size_t(s) >> 5] |= 1u << (s & 31);
    }
  }
  const int64_t pool_cap = 2 * int64_t(d->path_beam) * d->prefix_capacity + d->path_beam;
  if (pool_cap > 0x3fffffff || int64_t(2) * d->path_beam * d->prefix_capacity > 0x3fffffff)
    return fail(WEKWS_HIP_EINVAL, "ctc_kws: prefix_capacity %d too large", d->prefix_capacity);
  CtcKws* o = new (std::nothrow) CtcKws;
  if (!o) return fail(WEKWS_HIP_ENOMEM, "host allocation failed");
  o->device = d->device;
  DeviceGuard g(d->device);
  wekws::CtcParams& p = o->p;
  p.V = d->vocab; p.K = d->score_beam; p.PB = d->path_beam; p.cap = d->prefix_capacity; p.pool_cap = int(pool_cap);
  p.n_slots = d->max_streams; p.slot_bytes = wekws::ctc_slot_bytes(p.PB, p.cap, p.pool_cap);
  p.n_kw = d->num_keywords; p.threshold = d->threshold; p.min_frames = d->min_frames; p.max_frames = d->max_frames;
  p.interval_frames = d->interval_frames; p.ds = d->downsampling;
  hipError_t e = hipMalloc(&o->kw, kw.size() * 4);
  if (e == hipSuccess) e = hipMemcpy(o->kw, kw.data(), kw.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && !set.empty()) e = hipMalloc(&o->tokset, set.size() * 4);
  if (e == hipSuccess && !set.empty()) e = hipMemcpy(o->tokset, set.data(), set.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && p.n_slots > 0) e = hipMalloc(&o->slots, p.slot_bytes * size_t(p.n_slots));
  p.kw_off = o->kw; p.kw_tok = o->kw + d->num_keywords + 1; p.tokset = o->tokset; p.slots = o->slots;
  if (e == hipSuccess && p.n_slots > 0 && wekws::launch_ctc_kws_init(p, nullptr)) e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = hip_fail(e, "ctc_kws create");
    wekws_hip_ctc_kws_destroy(o);
    return rc;
  }
  *out = o;
  return WEKWS_HIP_OK;
}

void wekws_hip_ctc_kws_destroy(void* h) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o) return;
  DeviceGuard g(o->device);
  (void)hipDeviceSynchronize();
  if (o->slots) (void)hipFree(o->slots);
  if (o->tokset) (void)hipFree(o->tokset);
  if (o->kw) (void)hipFree(o->kw);
  if (o->ws) (void)hipFree(o->ws);
  delete o;
}

int wekws_hip_ctc_kws_step(void* h, const float* probs, int B, int T, const int32_t* stream_ids, const int32_t* frames,
                           wekws_hip_ctc_kws_result* results, void* stream) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (B < 0 || T < 0) return fail(WEKWS_HIP_EINVAL, "ctc_kws_step: B=%d T=%d", B, T);
  if (B == 0) return WEKWS_HIP_OK;
  if (!stream_ids || !results || (T > 0 && !probs)) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  DeviceGuard g(o->device);
  if (wekws::launch_ctc_kws(o->p, 0, probs, B, T, stream_ids, frames, reinterpret_cast<wekws::CtcResult*>(results), nullptr,
                            0, static_cast<hipStream_t>(stream)))
    return hip_fail(hipGetLastError(), "ctc_kws_step launch");
  return WEKWS_HIP_OK;
}

size_t wekws_hip_ctc_kws_beam_bytes(void* h, int cap) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o || cap < 1) return 0;
  return wekws::ctc_beam_bytes(o->p.PB, cap);
}

int wekws_hip_ctc_kws_search(void* h, const float* probs, int B, int T, const int32_t* lengths,
                             wekws_hip_ctc_kws_result* results, void* beams, void* stream) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (B < 0 || T < 0) return fail(WEKWS_HIP_EINVAL, "ctc_kws_search: B=%d T=%d", B, T);
  if (B == 0) return WEKWS_HIP_OK;
  if (!results || (T > 0 && !probs)) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  DeviceGuard g(o->device);
  wekws::CtcParams p = o->p;
  p.cap = T > 0 ? T : 1;                 // a prefix grows by at most one token per frame: never overflows
  p.pool_cap = p.PB * p.cap;             // at most PB new cells per frame: never compacts
  p.n_slots = B;
  p.slot_bytes = wekws::ctc_slot_bytes(p.PB, p.cap, p.pool_cap);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(o->mu);
  const size_t need = p.slot_bytes * size_t(B);
  if (need > o->ws_bytes) {
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess && o->ws) { e = hipFree(o->ws); o->ws = nullptr; o->ws_bytes = 0; }
    if (e == hipSuccess) e = hipMalloc(&o->ws, need);
    if (e != hipSuccess) return hip_fail(e, "ctc_kws_search workspace");
    o->ws_bytes = need;
  }
  p.slots = o->ws;
  if (wekws::launch_ctc_kws(p, 1, probs, B, T, nullptr, lengths, reinterpret_cast<wekws::CtcResult*>(results),
                            static_cast<char*>(beams), wekws::ctc_beam_bytes(p.PB, p.cap), s))
    return hip_fail(hipGetLastError(), "ctc_kws_search launch");
  return WEKWS_HIP_OK;
}

int wekws_hip_ctc_kws_reset(void* h, const int32_t* ids, int n, int all, void* stream) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (n < 0 || (n > 0 && !ids)) return fail(WEKWS_HIP_EINVAL, "ctc_kws_reset: n=%d", n);
  if (n == 0) return WEKWS_HIP_OK;
  DeviceGuard g(o->device);
  if (wekws::launch_ctc_kws_reset(o->p, ids, n, all, static_cast<hipStream_t>(stream)))
    return hip_fail(hipGetLastError(), "ctc_kws_reset launch");
  return WEKWS_HIP_OK;
}

int wekws_hip_ctc_kws_read_beam(void* h, int id, void* out, void* stream) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (id < 0 || id >= o->p.n_slots) return fail(WEKWS_HIP_EINVAL, "ctc_kws_read_beam: id %d outside 0..%d", id, o->p.n_slots - 1);
  DeviceGuard g(o->device);
  if (wekws::launch_ctc_kws_read_beam(o->p, id, static_cast<char*>(out), static_cast<hipStream_t>(stream)))
    return hip_fail(hipGetLastError(), "ctc_kws_read_beam launch");
  return WEKWS_HIP_OK;
}

int wekws_hip_ctc_kws_status(void* h, int id, int32_t* status_out, void* stream) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o || !status_out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (id < 0 || id >= o->p.n_slots) return fail(WEKWS_HIP_EINVAL, "ctc_kws_status: id %d outside 0..%d", id, o->p.n_slots - 1);
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const char* src = o->slots + size_t(id) * o->p.slot_bytes + offsetof(wekws::CtcSlotHead, status);
  hipError_t e = hipMemcpyAsync(status_out, src, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, "ctc_kws_status");
  return WEKWS_HIP_OK;
}

}  // extern "C"
