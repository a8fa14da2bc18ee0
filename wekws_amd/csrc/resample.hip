// Launcher, handle and C ABI of the resampler (resample.hip.h, resample_plan.h).
#include "resample.hip.h"

#include <cstring>
#include <new>

#include "host_util.h"

namespace wekws {

template <typename In, typename Out>
static int launch_one(const ResampleParams& P, size_t lds, const ResampleRow* rows, const void* x, int64_t xstride, int16_t* hist,
                      void* y, int B, int mcap, int max_grid, hipStream_t stream) {
  // (a capacity of 0 still takes one tile per row: a push without room for output moves the streams' history)
  const int tiles_per_row = mcap > 0 ? (mcap + kResampleTile - 1) / kResampleTile : 1;
  const int64_t total = int64_t(B) * tiles_per_row;
  if (total <= 0) return 0;
  const int64_t grid = total < max_grid ? total : max_grid;
  hipLaunchKernelGGL((resample_kernel<In, Out>), dim3(unsigned(grid)), dim3(kResampleTile), lds, stream, P, rows,
                     static_cast<const In*>(x), xstride, reinterpret_cast<In*>(hist), static_cast<Out*>(y), mcap, tiles_per_row, total);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_resample(const ResampleParams& P, size_t lds, int in_i16, int out_i16, const ResampleRow* rows, const void* x,
                    int64_t xstride, int16_t* hist, void* y, int B, int mcap, int max_grid, hipStream_t stream) {
  if (in_i16) return out_i16 ? launch_one<int16_t, int16_t>(P, lds, rows, x, xstride, hist, y, B, mcap, max_grid, stream)
                             : launch_one<int16_t, float>(P, lds, rows, x, xstride, hist, y, B, mcap, max_grid, stream);
  // (float rows have no history: the one-shot entry points alone take them)
  return out_i16 ? launch_one<float, int16_t>(P, lds, rows, x, xstride, nullptr, y, B, mcap, max_grid, stream)
                 : launch_one<float, float>(P, lds, rows, x, xstride, nullptr, y, B, mcap, max_grid, stream);
}

}  // namespace wekws

// ------------------------------------------------------------------------------------------------ C ABI
namespace {

typedef wekws_hip_resample Rs;

// the plan of a configuration, or the refusal: EINVAL for rates no resampler has, EUNSUPPORTED for a pair whose live table
// does not fit the LDS budget
int plan_cfg(const wekws_hip_resample_cfg* c, wekws::ResamplePlan* p) {
  if (c->orig_freq <= 0 || c->new_freq <= 0)
    return fail(WEKWS_HIP_EINVAL, "resample: orig_freq %d, new_freq %d: rates are positive", c->orig_freq, c->new_freq);
  if (c->out_dtype != WEKWS_HIP_RESAMPLE_OUT_F32 && c->out_dtype != WEKWS_HIP_RESAMPLE_OUT_I16)
    return fail(WEKWS_HIP_EINVAL, "resample: out_dtype %d", c->out_dtype);
  if (c->max_streams < 0 || (c->max_streams > 0 && c->max_chunk <= 0))
    return fail(WEKWS_HIP_EINVAL, "resample: max_streams=%d max_chunk=%d", c->max_streams, c->max_chunk);
  if (wekws::resample_plan_ranges(c->orig_freq, c->new_freq, c->lowpass_filter_width, c->rolloff, p))
    return fail(WEKWS_HIP_EINVAL, "resample: lowpass_filter_width %d, rolloff %g (a width >= 1, 0 < rolloff <= 1)",
                c->lowpass_filter_width, c->rolloff);
  const int64_t lds = wekws::resample_lds_bytes(*p);
  if (lds > wekws::kResampleLdsBudget || int64_t(p->n) * p->K > (int64_t(1) << 24))
    return fail(WEKWS_HIP_EUNSUPPORTED, "resample %d -> %d: %d phases x %d live taps and a tile of %lld samples need %lld bytes of LDS, "
                "the budget is %d", c->orig_freq, c->new_freq, p->n, p->max_live, (long long)wekws::resample_tile_cap(*p),
                (long long)lds, wekws::kResampleLdsBudget);
  return WEKWS_HIP_OK;
}

}  // namespace

extern "C" {

int64_t wekws_hip_resample_num_samples(int orig_freq, int new_freq, int64_t nsamp) {
  if (orig_freq <= 0 || new_freq <= 0 || nsamp < 0) {
    fail(WEKWS_HIP_EINVAL, "resample_num_samples: orig_freq=%d new_freq=%d nsamp=%lld", orig_freq, new_freq, (long long)nsamp);
    return -1;
  }
  wekws::ResamplePlan p;
  const int64_t g = wekws::resample_gcd(orig_freq, new_freq);
  p.o = int32_t(orig_freq / g); p.n = int32_t(new_freq / g);
  return wekws::resample_num_samples(p, nsamp);
}

void wekws_hip_resample_destroy(void* h) {
  Rs* o = static_cast<Rs*>(h);
  if (!o) return;
  DeviceGuard g(o->device);
  (void)hipDeviceSynchronize();
  for (int i = 0; i < wekws::kResampleRing; ++i) {
    if (o->ev[i]) (void)hipEventDestroy(o->ev[i]);
    if (o->h_rows[i]) (void)hipHostFree(o->h_rows[i]);
    if (o->d_rows[i]) (void)hipFree(o->d_rows[i]);
  }
  if (o->d_live) (void)hipFree(o->d_live);
  if (o->d_full) (void)hipFree(o->d_full);
  if (o->d_meta) (void)hipFree(o->d_meta);
  if (o->hist) (void)hipFree(o->hist);
  for (Rs::OnceSlot& t : o->once_ring) {
    if (t.ev) (void)hipEventDestroy(t.ev);
    if (t.h) (void)hipHostFree(t.h);
    if (t.d) (void)hipFree(t.d);
  }
  delete o;
}

int wekws_hip_resample_create(const wekws_hip_resample_cfg* cfg, void** out) {
  if (!cfg || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  wekws::ResamplePlan plan;
  if (int rc = plan_cfg(cfg, &plan)) return rc;
  const int hist_cap = (wekws::resample_hist_cap(plan) + 1) & ~1;
  if (int64_t(cfg->max_streams) * 2 * hist_cap > 0x7fffffffLL || int64_t(cfg->max_chunk) > 0x3fffffffLL)
    return fail(WEKWS_HIP_EINVAL, "resample: max_streams %d x max_chunk %d is out of range", cfg->max_streams, cfg->max_chunk);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev)
    return fail(WEKWS_HIP_EDEVICE, "device %d of %d", cfg->device, ndev);
  Rs* o = new (std::nothrow) Rs;
  if (!o) return fail(WEKWS_HIP_ENOMEM, "host allocation failed");
  wekws::resample_plan_taps(&plan);
  o->device = cfg->device;
  o->out_i16 = cfg->out_dtype == WEKWS_HIP_RESAMPLE_OUT_I16;
  o->max_streams = cfg->max_streams; o->max_chunk = cfg->max_chunk; o->hist_cap = hist_cap;
  const int n = plan.n, K = plan.K, stride = wekws::resample_stride(plan.max_live);
  std::vector<float> live(size_t(n) * stride, 0.f);
  std::vector<int32_t> meta(size_t(2) * n);
  for (int i = 0; i < n; ++i) {
    meta[size_t(i)] = plan.first[size_t(i)];
    meta[size_t(n) + i] = plan.last[size_t(i)] - plan.first[size_t(i)] + 1;
    for (int m = plan.first[size_t(i)]; m <= plan.last[size_t(i)]; ++m)
      live[size_t(i) * stride + (m - plan.first[size_t(i)])] = plan.taps[size_t(i) * K + m];
  }
  int64_t tile_off = 0;
  o->lds = size_t(wekws::resample_lds_bytes(plan, &tile_off));
  const size_t ns = size_t(cfg->max_streams);
  o->received.assign(ns, 0); o->emitted.assign(ns, 0); o->origin.assign(ns, 0);
  o->par.assign(ns, 0); o->seen.assign(ns, 0); o->flushed.assign(ns, 0);
  o->steps.reserve(ns);
  DeviceGuard g(cfg->device);
  hipError_t e = hipMalloc(&o->d_live, live.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(o->d_live, live.data(), live.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&o->d_full, plan.taps.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(o->d_full, plan.taps.data(), plan.taps.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&o->d_meta, meta.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemcpy(o->d_meta, meta.data(), meta.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess && ns > 0) e = hipMalloc(&o->hist, ns * 2 * size_t(hist_cap) * sizeof(int16_t));
  if (e == hipSuccess && ns > 0) e = hipMemset(o->hist, 0, ns * 2 * size_t(hist_cap) * sizeof(int16_t));
  for (int i = 0; i < wekws::kResampleRing && e == hipSuccess && ns > 0; ++i) {
    e = hipHostMalloc(&o->h_rows[i], ns * sizeof(wekws::ResampleRow), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&o->d_rows[i], ns * sizeof(wekws::ResampleRow));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&o->ev[i], hipEventDisableTiming);
  }
  hipDeviceProp_t prop;
  if (e == hipSuccess) e = hipGetDeviceProperties(&prop, cfg->device);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = hip_fail(e, "resample create");
    wekws_hip_resample_destroy(o);
    return rc;
  }
  o->max_grid = prop.multiProcessorCount > 0 ? prop.multiProcessorCount * 8 : 2048;
  o->P.o = plan.o; o->P.n = n; o->P.K = K; o->P.width = plan.width;
  o->P.stride = stride;
  o->P.tile_cap = int32_t(wekws::resample_tile_cap(plan));
  o->P.tile_off = int32_t(tile_off);
  o->P.live = o->d_live; o->P.first = o->d_meta; o->P.count = o->d_meta + n; o->P.full = o->d_full;
  o->plan = std::move(plan);
  *out = o;
  return WEKWS_HIP_OK;
}

int wekws_hip_resample_max_out(void* h, int nmax, int flush) {
  Rs* o = static_cast<Rs*>(h);
  if (!o || nmax < 0) return 0;
  const int64_t m = wekws::resample_max_out(o->plan, nmax, flush);
  return int(m > 0x7fffffffLL ? 0x7fffffffLL : m);
}

}  // extern "C"

namespace {

// one-shot: every row an utterance of nsamp[b] samples (NULL: nmax) from its first sample
int compute(void* h, const void* pcm, int in_i16, int B, int nmax, const int32_t* nsamp, void* out, int mcap, void* stream_) {
  Rs* o = static_cast<Rs*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (B < 0 || nmax < 0 || mcap < 0 || nmax > 0x3fffffff || mcap > 0x3fffffff)
    return fail(WEKWS_HIP_EINVAL, "resample_compute: B=%d nmax=%d mcap=%d", B, nmax, mcap);
  if (B == 0 || mcap == 0) {
    for (int b = 0; b < B; ++b)
      if (wekws::resample_num_samples(o->plan, nsamp ? nsamp[b] : nmax) > 0)
        return fail(WEKWS_HIP_EINVAL, "resample_compute: row %d yields samples, mcap is 0", b);
    return WEKWS_HIP_OK;
  }
  if (!out || (nmax > 0 && !pcm)) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(o->mu);
  o->once.clear();
  for (int b = 0; b < B; ++b) {
    const int len = nsamp ? nsamp[b] : nmax;
    if (len < 0 || len > nmax) return fail(WEKWS_HIP_EINVAL, "resample_compute: row %d: %d samples outside 0..%d", b, len, nmax);
    const int64_t cnt = wekws::resample_num_samples(o->plan, len);
    if (cnt > mcap) return fail(WEKWS_HIP_EINVAL, "resample_compute: row %d yields %lld samples, mcap is %d", b, (long long)cnt, mcap);
    wekws::ResampleRow R{};
    R.i0 = 0; R.base_rel = -o->plan.width; R.cnt = int32_t(cnt); R.h = 0; R.hi_valid = len;
    o->once.push_back(R);
  }
  // ---- the row table travels through a ring of pinned host tables with device twins, like a push's: calls queue back to back
  // without a synchronise; the host waits only for the call that used the slot kResampleRing calls ago.  A slot too small for
  // the call is replaced (behind that wait, so no launch still reads it).
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream_);
  Rs::OnceSlot& slot = o->once_ring[o->once_next];
  if (slot.used) {
    const hipError_t e = hipEventSynchronize(slot.ev);
    if (e != hipSuccess) return hip_fail(e, "resample_compute: table ring");
    slot.used = false;
  }
  if (size_t(B) > slot.cap) {
    if (stream_is_capturing(s)) return fail(WEKWS_HIP_EINVAL, "resample_compute: %d rows need a larger table: not inside a capture", B);
    if (slot.h) (void)hipHostFree(slot.h);
    if (slot.d) (void)hipFree(slot.d);
    slot.h = nullptr; slot.d = nullptr; slot.cap = 0;
    HIP_TRY(hipHostMalloc(&slot.h, size_t(B) * sizeof(wekws::ResampleRow), hipHostMallocDefault));
    HIP_TRY(hipMalloc(&slot.d, size_t(B) * sizeof(wekws::ResampleRow)));
    if (!slot.ev) HIP_TRY(hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming));
    slot.cap = size_t(B);
  }
  o->once_next = (o->once_next + 1) % wekws::kResampleRing;
  std::memcpy(slot.h, o->once.data(), size_t(B) * sizeof(wekws::ResampleRow));
  HIP_TRY(hipMemcpyAsync(slot.d, slot.h, size_t(B) * sizeof(wekws::ResampleRow), hipMemcpyHostToDevice, s));
  const int rc = wekws::launch_resample(o->P, o->lds, in_i16, o->out_i16, slot.d, pcm, nmax, nullptr, out, B, mcap, o->max_grid, s);
  const hipError_t e = hipEventRecord(slot.ev, s);
  slot.used = e == hipSuccess;
  if (rc) return hip_fail(hipGetLastError(), "resample_compute launch");
  if (e != hipSuccess) return hip_fail(e, "resample_compute: event");
  return WEKWS_HIP_OK;
}

}  // namespace

extern "C" {

int wekws_hip_resample_compute(void* h, const float* pcm, int B, int nmax, const int32_t* nsamp, void* out, int mcap, void* stream) {
  return compute(h, pcm, 0, B, nmax, nsamp, out, mcap, stream);
}

int wekws_hip_resample_compute_i16(void* h, const int16_t* pcm, int B, int nmax, const int32_t* nsamp, void* out, int mcap,
                                   void* stream) {
  return compute(h, pcm, 1, B, nmax, nsamp, out, mcap, stream);
}

int wekws_hip_resample_push(void* h, const int16_t* pcm, int B, int nmax, const int32_t* stream_ids, const int32_t* nsamp, int flush,
                            void* out, int mcap, int32_t* counts, void* stream_) {
  Rs* o = static_cast<Rs*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (B < 0 || nmax < 0 || mcap < 0) return fail(WEKWS_HIP_EINVAL, "resample_push: B=%d nmax=%d mcap=%d", B, nmax, mcap);
  if (B == 0) return WEKWS_HIP_OK;
  if (!stream_ids || !nsamp || !counts || (nmax > 0 && !pcm)) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (o->max_streams < 1) return fail(WEKWS_HIP_EINVAL, "resample_push: the handle was created without streams (max_streams 0)");
  if (nmax > o->max_chunk) return fail(WEKWS_HIP_EINVAL, "resample_push: nmax %d > max_chunk %d", nmax, o->max_chunk);
  if (B > o->max_streams) return fail(WEKWS_HIP_EINVAL, "resample_push: %d rows for %d streams", B, o->max_streams);
  if (int64_t(B) * mcap > (int64_t(1) << 40)) return fail(WEKWS_HIP_EINVAL, "resample_push: B %d x mcap %d is out of range", B, mcap);
  std::lock_guard<std::mutex> lk(o->mu);
  // ---- the whole call is planned first: a refusal launches nothing and changes no stream.  (epoch / seen are scratch of this
  // planning pass -- which ids the call has named so far -- and carry nothing from one call to the next: a refused call may
  // leave them advanced.)
  if (++o->epoch == 0x7fffffff) { o->epoch = 1; o->seen.assign(o->seen.size(), 0); }
  o->steps.clear();
  int64_t need_cap = 0;
  for (int b = 0; b < B; ++b) {
    const int id = stream_ids[b];
    if (id < 0 || id >= o->max_streams) return fail(WEKWS_HIP_EINVAL, "resample_push: row %d: stream %d outside 0..%d", b, id, o->max_streams - 1);
    if (o->seen[id] == o->epoch) return fail(WEKWS_HIP_EINVAL, "resample_push: row %d: stream %d is given twice", b, id);
    o->seen[id] = o->epoch;
    if (nsamp[b] < 0 || nsamp[b] > nmax) return fail(WEKWS_HIP_EINVAL, "resample_push: row %d: %d samples outside 0..%d", b, nsamp[b], nmax);
    if (o->flushed[id]) return fail(WEKWS_HIP_EINVAL, "resample_push: row %d: stream %d was flushed; reset it first", b, id);
    const wekws::ResampleStep st = wekws::resample_step(o->plan, o->received[id], nsamp[b], flush);
    const int64_t N2 = o->received[id] + nsamp[b];
    if (N2 - st.keep_from > o->hist_cap || st.keep_from < o->origin[id] || st.total < o->emitted[id])
      return fail(WEKWS_HIP_EINVAL, "resample_push: internal: plan outside the handle's buffers");
    if (st.total - o->emitted[id] > need_cap) need_cap = st.total - o->emitted[id];
    o->steps.push_back(st);
  }
  if (need_cap > mcap) return fail(WEKWS_HIP_EINVAL, "resample_push: a row yields %lld samples, mcap is %d", (long long)need_cap, mcap);
  if (mcap > 0 && !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  // ---- the plan table, in stream order
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream_);
  const int slot = o->next;
  o->next = (slot + 1) % wekws::kResampleRing;
  if (o->ev_used[slot]) {
    const hipError_t e = hipEventSynchronize(o->ev[slot]);
    if (e != hipSuccess) return hip_fail(e, "resample_push: plan ring");
  }
  wekws::ResampleRow* rows = o->h_rows[slot];
  const wekws::ResamplePlan& p = o->plan;
  for (int b = 0; b < B; ++b) {
    const int id = stream_ids[b];
    const wekws::ResampleStep& st = o->steps[size_t(b)];
    const int64_t q0 = o->emitted[id], j0 = q0 / p.n, s0 = o->origin[id];
    wekws::ResampleRow& R = rows[b];
    R = wekws::ResampleRow{};
    R.i0 = int32_t(q0 - j0 * p.n);
    R.base_rel = int32_t(j0 * p.o - p.width - s0);
    R.cnt = int32_t(st.total - q0);
    R.h = int32_t(o->received[id] - s0);
    R.hi_valid = R.h + nsamp[b];
    R.hist_old = (id * 2 + o->par[id]) * o->hist_cap;
    R.hist_new = (id * 2 + (o->par[id] ^ 1)) * o->hist_cap;
    R.keep_from = int32_t(st.keep_from - s0);
    R.keep_cnt = int32_t(o->received[id] + nsamp[b] - st.keep_from);
  }
  hipError_t e = hipMemcpyAsync(o->d_rows[slot], rows, size_t(B) * sizeof(wekws::ResampleRow), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_fail(e, "resample_push: plan upload");
  // ---- one launch; from here the streams' state moves
  const int rc = wekws::launch_resample(o->P, o->lds, 1, o->out_i16, o->d_rows[slot], pcm, nmax, o->hist, out, B, mcap, o->max_grid, s);
  e = hipEventRecord(o->ev[slot], s);
  o->ev_used[slot] = e == hipSuccess;
  for (int b = 0; b < B; ++b) {
    const int id = stream_ids[b];
    const wekws::ResampleStep& st = o->steps[size_t(b)];
    counts[b] = int32_t(st.total - o->emitted[id]);
    o->received[id] += nsamp[b];
    o->emitted[id] = st.total;
    o->origin[id] = st.keep_from;
    o->par[id] ^= 1;
    if (flush) o->flushed[id] = 1;
  }
  if (rc) return hip_fail(hipGetLastError(), "resample_push launch");
  if (e != hipSuccess) return hip_fail(e, "resample_push: event");
  return WEKWS_HIP_OK;
}

int wekws_hip_resample_reset(void* h, const int32_t* ids, int n) {
  Rs* o = static_cast<Rs*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (n < 0 || (n > 0 && !ids)) return fail(WEKWS_HIP_EINVAL, "resample_reset: n=%d", n);
  std::lock_guard<std::mutex> lk(o->mu);
  for (int i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= o->max_streams)
      return fail(WEKWS_HIP_EINVAL, "resample_reset: stream %d outside 0..%d", ids[i], o->max_streams - 1);
  // the counts ARE the state: a stream that has received nothing reads nothing of its device buffers
  for (int i = 0; i < n; ++i) {
    const int id = ids[i];
    o->received[id] = 0; o->emitted[id] = 0; o->origin[id] = 0; o->flushed[id] = 0;
  }
  return WEKWS_HIP_OK;
}

int wekws_hip_resample_counts(void* h, int id, int64_t counts_out[4]) {
  Rs* o = static_cast<Rs*>(h);
  if (!o || !counts_out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (id < 0 || id >= o->max_streams) return fail(WEKWS_HIP_EINVAL, "resample_counts: stream %d outside 0..%d", id, o->max_streams - 1);
  std::lock_guard<std::mutex> lk(o->mu);
  counts_out[0] = o->received[id]; counts_out[1] = o->emitted[id];
  counts_out[2] = o->received[id] - o->origin[id]; counts_out[3] = o->flushed[id];
  return WEKWS_HIP_OK;
}

}  // extern "C"
