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

int launch_ctc_kws_assign(const CtcParams& p, int32_t* slot_set, const int32_t* ids, const int32_t* sets, int n, hipStream_t stream) {
  hipLaunchKernelGGL(ctc_kws_assign_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, p, slot_set, ids, sets, n);
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
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "host_util.h"

namespace {

// A device table that grows by copy.  Launches take the pointer by value, so a launch enqueued before the table grew keeps
// reading the allocation it was given: the outgrown one is retired, not freed, until destroy.  Capacities double, so the
// retired copies of a table total less than the live one.
struct DevTable {
  char* p = nullptr;
  size_t cap = 0;   // bytes
};

// Pinned host memory for what a set operation uploads (and, where a kernel reads the upload -- assign --, device memory of
// the same size); an event says when the stream is done with both.  A small ring, so that a few operations can be in flight.
constexpr int kCtcStageRing = 4;
struct Stage {
  char* h = nullptr;
  char* d = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  bool used = false;
};

struct CtcKws {
  int device = 0;
  wekws::CtcParams p{};   // the streaming slots; the table pointers change under tab_mu
  char* slots = nullptr;
  int32_t* slot_set = nullptr;
  std::mutex tab_mu;      // the keyword sets: the host table, the device tables, the staging ring
  wekws::CtcSetTable tab;
  DevTable d_recs, d_kw, d_mask;
  std::vector<void*> retired;
  Stage stage[kCtcStageRing];
  int next = 0;
  std::mutex mu;          // the offline workspace
  char* ws = nullptr;
  size_t ws_bytes = 0;
};

wekws::CtcParams params_of(CtcKws* o) {
  std::lock_guard<std::mutex> lk(o->tab_mu);
  return o->p;
}

// make the table hold `need` bytes; what it held is copied over on `s`
hipError_t grow(CtcKws* o, DevTable& t, size_t need, hipStream_t s) {
  if (need <= t.cap) return hipSuccess;
  size_t cap = t.cap ? 2 * t.cap : 1024;
  while (cap < need) cap *= 2;
  char* n = nullptr;
  hipError_t e = hipMalloc(&n, cap);
  if (e != hipSuccess) return e;
  if (t.p) {
    e = hipMemcpyAsync(n, t.p, t.cap, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) { (void)hipFree(n); return e; }
    o->retired.push_back(t.p);
  }
  t.p = n; t.cap = cap;
  return hipSuccess;
}

// room for the tables' images as they are now; the launch parameters follow
hipError_t fit_tables(CtcKws* o, hipStream_t s) {
  hipError_t e = grow(o, o->d_recs, o->tab.recs.size() * sizeof(wekws::CtcSetRec), s);
  if (e == hipSuccess) e = grow(o, o->d_kw, o->tab.kw.size() * 4, s);
  if (e == hipSuccess) e = grow(o, o->d_mask, o->tab.mask.size() * 4, s);
  o->p.sets = reinterpret_cast<const wekws::CtcSetRec*>(o->d_recs.p);
  o->p.kw_arena = reinterpret_cast<const int32_t*>(o->d_kw.p);
  o->p.mask_arena = reinterpret_cast<const uint32_t*>(o->d_mask.p);
  return e;
}

// the next staging buffer of the ring, free again and at least `bytes` large; `device`: with its device half
hipError_t stage_get(CtcKws* o, size_t bytes, bool device, Stage** out) {
  Stage& st = o->stage[o->next];
  o->next = (o->next + 1) % kCtcStageRing;
  hipError_t e = hipSuccess;
  if (st.used) { e = hipEventSynchronize(st.ev); st.used = false; }
  if (e == hipSuccess && !st.ev) e = hipEventCreateWithFlags(&st.ev, hipEventDisableTiming);
  if (e == hipSuccess && bytes > st.cap) {
    if (st.h) (void)hipHostFree(st.h);
    if (st.d) (void)hipFree(st.d);
    st.h = st.d = nullptr; st.cap = 0;
    size_t cap = 4096;
    while (cap < bytes) cap *= 2;
    e = hipHostMalloc(reinterpret_cast<void**>(&st.h), cap, hipHostMallocDefault);
    if (e == hipSuccess) st.cap = cap;
  }
  if (e == hipSuccess && device && !st.d) e = hipMalloc(&st.d, st.cap);
  *out = &st;
  return e;
}
hipError_t stage_done(Stage* st, hipStream_t s) {
  const hipError_t e = hipEventRecord(st->ev, s);
  st->used = e == hipSuccess;
  return e;
}

// the record, the keyword block and the mask of set `id` from the host table to the device tables, on `s`
hipError_t upload_set(CtcKws* o, int id, hipStream_t s) {
  const wekws::CtcSetRec r = o->tab.recs[size_t(id)];
  const size_t nk = size_t(o->tab.kw_len(id)) * 4, nm = r.mask_word >= 0 ? size_t(o->tab.W) * 4 : 0;
  Stage* st = nullptr;
  hipError_t e = stage_get(o, nk + nm + sizeof r, false, &st);
  if (e != hipSuccess) return e;
  std::memcpy(st->h, o->tab.kw.data() + r.kw_base, nk);
  if (nm) std::memcpy(st->h + nk, o->tab.mask.data() + r.mask_word, nm);
  std::memcpy(st->h + nk + nm, &r, sizeof r);
  e = hipMemcpyAsync(o->d_kw.p + size_t(r.kw_base) * 4, st->h, nk, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && nm) e = hipMemcpyAsync(o->d_mask.p + size_t(r.mask_word) * 4, st->h + nk, nm, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(o->d_recs.p + size_t(id) * sizeof r, st->h + nk + nm, sizeof r, hipMemcpyHostToDevice, s);
  const hipError_t e2 = stage_done(st, s);
  return e != hipSuccess ? e : e2;
}

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
  CtcKws* o = new (std::nothrow) CtcKws;
  if (!o) return fail(WEKWS_HIP_ENOMEM, "host allocation failed");
  // set 0: the descriptor's keywords, token set and threshold
  char why[256];
  o->tab.init(d->vocab, d->max_streams);
  if (o->tab.add(wekws::CtcSetSpec{d->keyword_tokens, d->keyword_offsets, d->num_keywords, d->token_set, d->token_set_len, d->threshold},
                 why, sizeof why) != 0) {
    delete o;
    return fail(WEKWS_HIP_EINVAL, "ctc_kws: %s", why);
  }
  const int64_t pool_cap = 2 * int64_t(d->path_beam) * d->prefix_capacity + d->path_beam;
  if (pool_cap > 0x3fffffff || int64_t(2) * d->path_beam * d->prefix_capacity > 0x3fffffff) {
    delete o;
    return fail(WEKWS_HIP_EINVAL, "ctc_kws: prefix_capacity %d too large", d->prefix_capacity);
  }
  o->device = d->device;
  DeviceGuard g(d->device);
  wekws::CtcParams& p = o->p;
  p.V = d->vocab; p.K = d->score_beam; p.PB = d->path_beam; p.cap = d->prefix_capacity; p.pool_cap = int(pool_cap);
  p.n_slots = d->max_streams; p.slot_bytes = wekws::ctc_slot_bytes(p.PB, p.cap, p.pool_cap);
  p.n_sets = 1; p.min_frames = d->min_frames; p.max_frames = d->max_frames;
  p.interval_frames = d->interval_frames; p.ds = d->downsampling;
  hipError_t e = fit_tables(o, nullptr);
  if (e == hipSuccess) e = hipMemcpy(o->d_recs.p, o->tab.recs.data(), sizeof(wekws::CtcSetRec), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(o->d_kw.p, o->tab.kw.data(), o->tab.kw.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && !o->tab.mask.empty()) e = hipMemcpy(o->d_mask.p, o->tab.mask.data(), o->tab.mask.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && p.n_slots > 0) e = hipMalloc(&o->slots, p.slot_bytes * size_t(p.n_slots));
  if (e == hipSuccess && p.n_slots > 0) e = hipMalloc(&o->slot_set, size_t(p.n_slots) * 4);
  if (e == hipSuccess && p.n_slots > 0) e = hipMemset(o->slot_set, 0, size_t(p.n_slots) * 4);
  p.slots = o->slots; p.slot_set = o->slot_set;
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
  if (o->slot_set) (void)hipFree(o->slot_set);
  for (DevTable* t : {&o->d_recs, &o->d_kw, &o->d_mask})
    if (t->p) (void)hipFree(t->p);
  for (void* r : o->retired) (void)hipFree(r);
  for (Stage& st : o->stage) {
    if (st.h) (void)hipHostFree(st.h);
    if (st.d) (void)hipFree(st.d);
    if (st.ev) (void)hipEventDestroy(st.ev);
  }
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
  if (wekws::launch_ctc_kws(params_of(o), 0, probs, B, T, stream_ids, frames, reinterpret_cast<wekws::CtcResult*>(results), nullptr,
                            0, static_cast<hipStream_t>(stream)))
    return hip_fail(hipGetLastError(), "ctc_kws_step launch");
  return WEKWS_HIP_OK;
}

size_t wekws_hip_ctc_kws_beam_bytes(void* h, int cap) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o || cap < 1) return 0;
  return wekws::ctc_beam_bytes(o->p.PB, cap);
}

int wekws_hip_ctc_kws_search_sets(void* h, const float* probs, int B, int T, const int32_t* lengths, const int32_t* sets,
                                  wekws_hip_ctc_kws_result* results, void* beams, void* stream) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (B < 0 || T < 0) return fail(WEKWS_HIP_EINVAL, "ctc_kws_search: B=%d T=%d", B, T);
  if (B == 0) return WEKWS_HIP_OK;
  if (!results || (T > 0 && !probs)) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(o->mu);
  wekws::CtcParams p;
  {
    std::lock_guard<std::mutex> tl(o->tab_mu);
    for (int b = 0; sets && b < B; ++b)
      if (!o->tab.known(sets[b])) return fail(WEKWS_HIP_EINVAL, "ctc_kws_search_sets: row %d: set %d is not registered", b, sets[b]);
    p = o->p;
  }
  p.cap = T > 0 ? T : 1;                 // a prefix grows by at most one token per frame: never overflows
  p.pool_cap = p.PB * p.cap;             // at most PB new cells per frame: never compacts
  p.n_slots = B;
  p.slot_bytes = wekws::ctc_slot_bytes(p.PB, p.cap, p.pool_cap);
  const size_t slots_bytes = p.slot_bytes * size_t(B), need = slots_bytes + wekws::ctc_align(size_t(B) * 4);
  hipError_t e = hipSuccess;
  if (need > o->ws_bytes) {
    e = hipStreamSynchronize(s);
    if (e == hipSuccess && o->ws) { e = hipFree(o->ws); o->ws = nullptr; o->ws_bytes = 0; }
    if (e == hipSuccess) e = hipMalloc(&o->ws, need);
    if (e == hipSuccess) o->ws_bytes = need;
  }
  p.slots = o->ws;
  p.slot_set = nullptr;
  if (e == hipSuccess && sets) {       // the rows' set ids behind the slots
    std::lock_guard<std::mutex> tl(o->tab_mu);
    Stage* st = nullptr;
    e = stage_get(o, size_t(B) * 4, false, &st);
    if (e == hipSuccess) {
      std::memcpy(st->h, sets, size_t(B) * 4);
      p.slot_set = reinterpret_cast<const int32_t*>(o->ws + slots_bytes);
      e = hipMemcpyAsync(o->ws + slots_bytes, st->h, size_t(B) * 4, hipMemcpyHostToDevice, s);
      const hipError_t e2 = stage_done(st, s);
      if (e == hipSuccess) e = e2;
    }
  }
  if (e != hipSuccess) return hip_fail(e, "ctc_kws_search workspace");
  if (wekws::launch_ctc_kws(p, 1, probs, B, T, nullptr, lengths, reinterpret_cast<wekws::CtcResult*>(results),
                            static_cast<char*>(beams), wekws::ctc_beam_bytes(p.PB, p.cap), s))
    return hip_fail(hipGetLastError(), "ctc_kws_search launch");
  return WEKWS_HIP_OK;
}

int wekws_hip_ctc_kws_search(void* h, const float* probs, int B, int T, const int32_t* lengths,
                             wekws_hip_ctc_kws_result* results, void* beams, void* stream) {
  return wekws_hip_ctc_kws_search_sets(h, probs, B, T, lengths, nullptr, results, beams, stream);
}

int wekws_hip_ctc_kws_add_set(void* h, const int32_t* keyword_tokens, const int32_t* keyword_offsets, int num_keywords,
                              const int32_t* token_set, int token_set_len, double threshold, int32_t* set_out, void* stream) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (!set_out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  char why[256];
  std::lock_guard<std::mutex> lk(o->tab_mu);
  const int id = o->tab.add(wekws::CtcSetSpec{keyword_tokens, keyword_offsets, num_keywords, token_set, token_set_len, threshold}, why,
                            sizeof why);
  if (id < 0) return fail(WEKWS_HIP_EINVAL, "ctc_kws_add_set: %s", why);
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = fit_tables(o, s);
  if (e == hipSuccess) e = upload_set(o, id, s);
  if (e != hipSuccess) {
    (void)o->tab.drop(id, why, sizeof why);
    return hip_fail(e, "ctc_kws_add_set");
  }
  o->p.n_sets = int(o->tab.recs.size());
  *set_out = id;
  return WEKWS_HIP_OK;
}

int wekws_hip_ctc_kws_drop_set(void* h, int32_t set, void* stream) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  (void)stream;   // nothing on the device changes: no stream reads the set, and its id and room are written again by add_set
  char why[256];
  std::lock_guard<std::mutex> lk(o->tab_mu);
  if (o->tab.drop(set, why, sizeof why)) return fail(WEKWS_HIP_EINVAL, "ctc_kws_drop_set: %s", why);
  return WEKWS_HIP_OK;
}

int wekws_hip_ctc_kws_assign(void* h, const int32_t* ids, const int32_t* sets, int n, void* stream) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  char why[256];
  std::lock_guard<std::mutex> lk(o->tab_mu);
  if (o->tab.assign_check(ids, sets, n, why, sizeof why)) return fail(WEKWS_HIP_EINVAL, "ctc_kws_assign: %s", why);
  if (n == 0) return WEKWS_HIP_OK;
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  Stage* st = nullptr;
  hipError_t e = stage_get(o, size_t(n) * 8, true, &st);
  if (e != hipSuccess) return hip_fail(e, "ctc_kws_assign: staging");
  std::memcpy(st->h, ids, size_t(n) * 4);
  std::memcpy(st->h + size_t(n) * 4, sets, size_t(n) * 4);
  e = hipMemcpyAsync(st->d, st->h, size_t(n) * 8, hipMemcpyHostToDevice, s);
  int rc = 0;
  if (e == hipSuccess) {
    const int32_t* d = reinterpret_cast<const int32_t*>(st->d);
    rc = wekws::launch_ctc_kws_assign(o->p, o->slot_set, d, d + n, n, s);
  }
  const hipError_t e2 = stage_done(st, s);
  if (e != hipSuccess) return hip_fail(e, "ctc_kws_assign: upload");
  if (rc) return hip_fail(hipGetLastError(), "ctc_kws_assign launch");
  o->tab.assign_commit(ids, sets, n);
  if (e2 != hipSuccess) return hip_fail(e2, "ctc_kws_assign: event");
  return WEKWS_HIP_OK;
}

int wekws_hip_ctc_kws_stream_set(void* h, int id) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  std::lock_guard<std::mutex> lk(o->tab_mu);
  return o->tab.set_of(id);
}

int wekws_hip_ctc_kws_reset(void* h, const int32_t* ids, int n, int all, void* stream) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (n < 0 || (n > 0 && !ids)) return fail(WEKWS_HIP_EINVAL, "ctc_kws_reset: n=%d", n);
  if (n == 0) return WEKWS_HIP_OK;
  DeviceGuard g(o->device);
  if (wekws::launch_ctc_kws_reset(params_of(o), ids, n, all, static_cast<hipStream_t>(stream)))
    return hip_fail(hipGetLastError(), "ctc_kws_reset launch");
  return WEKWS_HIP_OK;
}

int wekws_hip_ctc_kws_read_beam(void* h, int id, void* out, void* stream) {
  CtcKws* o = static_cast<CtcKws*>(h);
  if (!o || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (id < 0 || id >= o->p.n_slots) return fail(WEKWS_HIP_EINVAL, "ctc_kws_read_beam: id %d outside 0..%d", id, o->p.n_slots - 1);
  DeviceGuard g(o->device);
  if (wekws::launch_ctc_kws_read_beam(params_of(o), id, static_cast<char*>(out), static_cast<hipStream_t>(stream)))
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
