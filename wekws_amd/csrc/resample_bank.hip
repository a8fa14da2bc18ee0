// Launcher of the rate bank's kernel (resample_bank.hip.h), the host core of BOTH resampler handles -- wekws_hip_resample_* is a bank
// of one S16 member that launches the single-rate kernel (resample.hip) -- and the C ABI of wekws_hip_resample_bank_*.  What a call
// does to the streams is planned in resample_streams.h; this unit words the refusals, owns the device memory and launches.
#include "resample_bank.hip.h"

#include <cstring>
#include <new>

#include "host_util.h"

namespace wekws {

template <typename Chunk, typename Out>
static int launch_bank_one(const ResampleParams* members, size_t lds, const ResampleRow* rows, const void* x, int64_t xstride,
                           int16_t* hist, void* y, int B, int mcap, int max_grid, hipStream_t stream) {
  // (a capacity of 0 still takes one tile per row: a push without room for output moves the streams' history)
  const int tiles_per_row = mcap > 0 ? (mcap + kResampleTile - 1) / kResampleTile : 1;
  const int64_t total = resample_bank_total(B, tiles_per_row);
  if (total <= 0) return 0;
  const int64_t grid = resample_bank_grid(total, max_grid);
  hipLaunchKernelGGL((resample_bank_kernel<Chunk, Out>), dim3(unsigned(grid)), dim3(kResampleTile), lds, stream, members, rows,
                     static_cast<const typename Chunk::Src*>(x), xstride, reinterpret_cast<typename Chunk::Sample*>(hist),
                     static_cast<Out*>(y), mcap, tiles_per_row, total);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_resample_bank(const ResampleParams* members, size_t lds, int source, int out_i16, const ResampleRow* rows, const void* x,
                         int64_t xstride, int16_t* hist, void* y, int B, int mcap, int max_grid, hipStream_t stream) {
  typedef ResampleChunk<int16_t> I16;
  typedef ResampleChunk<float> F32;
  if (source == kResampleBankWireBytes)
    return out_i16 ? launch_bank_one<ResampleWireChunk, int16_t>(members, lds, rows, x, xstride, hist, y, B, mcap, max_grid, stream)
                   : launch_bank_one<ResampleWireChunk, float>(members, lds, rows, x, xstride, hist, y, B, mcap, max_grid, stream);
  if (source == kResampleBankI16)
    return out_i16 ? launch_bank_one<I16, int16_t>(members, lds, rows, x, xstride, hist, y, B, mcap, max_grid, stream)
                   : launch_bank_one<I16, float>(members, lds, rows, x, xstride, hist, y, B, mcap, max_grid, stream);
  // (float rows have no history: the one-shot entry points alone take them)
  return out_i16 ? launch_bank_one<F32, int16_t>(members, lds, rows, x, xstride, nullptr, y, B, mcap, max_grid, stream)
                 : launch_bank_one<F32, float>(members, lds, rows, x, xstride, nullptr, y, B, mcap, max_grid, stream);
}

}  // namespace wekws

// ------------------------------------------------------------------------------------------------ the host core
namespace {

typedef wekws_hip_resample Rs;

// the entry point a message is prefixed with: [kind][push][wire call]
const char* const kEntry[2][2][2] = {{{"resample_compute", "resample_compute_wire"}, {"resample_push", "resample_push_wire"}},
                                     {{"resample_bank_compute", "resample_bank_compute_wire"},
                                      {"resample_bank_push", "resample_bank_push_wire"}}};

const char* wire_name(int enc) {
  static const char* const names[wekws::kWireCount] = {"s16", "mulaw", "alaw", "u8", "f32"};
  return enc >= 0 && enc < wekws::kWireCount ? names[enc] : "?";
}

int hip_fail_at(hipError_t e, const char* what, const char* step) {
  return fail(hip_code(e), "%s%s: %s", what, step, hipGetErrorString(e));
}

int check_cfg_fields(const char* name, const wekws_hip_resample_cfg* c) {
  if (c->out_dtype != WEKWS_HIP_RESAMPLE_OUT_F32 && c->out_dtype != WEKWS_HIP_RESAMPLE_OUT_I16)
    return fail(WEKWS_HIP_EINVAL, "%s: out_dtype %d", name, c->out_dtype);
  if (c->max_streams < 0 || (c->max_streams > 0 && c->max_chunk <= 0))
    return fail(WEKWS_HIP_EINVAL, "%s: max_streams=%d max_chunk=%d", name, c->max_streams, c->max_chunk);
  return WEKWS_HIP_OK;
}

// The plan of a configuration, or the refusal: EINVAL for a bank or rates no resampler has, EUNSUPPORTED for a member whose live
// table does not fit the LDS budget.  encs: NULL for every member S16 (a repeated rate is then the repeated pair).
// (A single-rate handle has its cfg's fields checked before its rates are planned and a bank after: each as it always was, so a cfg
// with two faults is refused with the code it always was.)
int plan_cfg(int kind, const wekws_hip_resample_cfg* c, const int32_t* rates, const int32_t* encs, int num, wekws::ResampleBankPlan* bp) {
  const bool single = kind == Rs::kSingle;
  const char* const name = single ? "resample" : "resample_bank";
  if (single)
    if (int rc = check_cfg_fields(name, c)) return rc;
  int bad = -1;
  const wekws::ResampleBankRefusal r =
      wekws::resample_bank_plan(rates, encs, num, c->new_freq, c->lowpass_filter_width, c->rolloff, bp, &bad);
  char who[48];                                                // a single-rate handle has no member to name
  if (single) snprintf(who, sizeof who, "%s", name);
  else snprintf(who, sizeof who, "%s: member %d", name, bad);
  switch (r) {
    case wekws::kResampleBankOk: break;
    case wekws::kResampleBankWire:
      return fail(WEKWS_HIP_EINVAL, "%s: encoding %d is none of s16, mulaw, alaw, u8, f32 (0..%d)", who, encs[bad], wekws::kWireCount - 1);
    case wekws::kResampleBankCount:
      return fail(WEKWS_HIP_EINVAL, "%s: %d rates: a bank holds 1..%d", name, num, wekws::kResampleBankMax);
    case wekws::kResampleBankRate:
      return fail(WEKWS_HIP_EINVAL, "%s: orig_freq %d, new_freq %d: rates are positive", who, bad >= 0 ? rates[bad] : 0, c->new_freq);
    case wekws::kResampleBankRepeat:
      if (encs) return fail(WEKWS_HIP_EINVAL, "%s repeats the pair (%d, %s)", who, rates[bad], wire_name(encs[bad]));
      return fail(WEKWS_HIP_EINVAL, "%s repeats the rate %d", who, rates[bad]);
    case wekws::kResampleBankParams:
      return fail(WEKWS_HIP_EINVAL, "%s: lowpass_filter_width %d, rolloff %g (a width >= 1, 0 < rolloff <= 1)", name,
                  c->lowpass_filter_width, c->rolloff);
    case wekws::kResampleBankLds: {
      const wekws::ResamplePlan& p = bp->members[size_t(bad)];
      return fail(WEKWS_HIP_EUNSUPPORTED, "%s, %d -> %d: %d phases x %d live taps and a tile of %lld samples need %lld bytes of LDS, "
                  "the budget is %d", who, rates[bad], c->new_freq, p.n, p.max_live, (long long)wekws::resample_tile_cap(p),
                  (long long)wekws::resample_lds_bytes(p), wekws::kResampleLdsBudget);
    }
  }
  if (single) return WEKWS_HIP_OK;
  if (c->orig_freq != rates[0])
    return fail(WEKWS_HIP_EINVAL, "resample_bank: cfg.orig_freq %d is not member 0's rate %d", c->orig_freq, rates[0]);
  return check_cfg_fields(name, c);
}

// The rows of a call (resample_bank_plan.h: resample_bank_check_rows) refused with r, in words.  width: nmax, or row_bytes of a
// wire call; limit: the most samples of a row.
int fail_rows(const wekws::ResampleBankPlan& bp, wekws::ResampleBankRowRefusal r, int bad, const char* what, int wire_call, const void* pcm,
              int width, const int32_t* nsamp, const int32_t* members, int64_t limit) {
  switch (r) {
    case wekws::kResampleRowsOk: break;
    case wekws::kResampleRowsAlign:
      return fail(WEKWS_HIP_EINVAL, "%s: pcm %p is not %d-byte aligned", what, pcm, wekws::kResampleWireAlign);
    case wekws::kResampleRowsWidth:
      return fail(WEKWS_HIP_EINVAL, "%s: row_bytes %d: a multiple of %d in 0..2^30-4", what, width, wekws::kResampleWireAlign);
    case wekws::kResampleRowsMember:
      return fail(WEKWS_HIP_EINVAL, "%s: row %d: member %d outside 0..%d", what, bad, members[bad], int(bp.members.size()) - 1);
    case wekws::kResampleRowsEncoding:
      return fail(WEKWS_HIP_EINVAL, "%s: row %d: member %d arrives as %s, not as s16: its rows go through the _wire calls", what, bad,
                  members[bad], wire_name(bp.wire[size_t(members[bad])]));
    case wekws::kResampleRowsLength: {
      const int64_t holds = wekws::resample_bank_row_samples(bp, wire_call, members[bad], width);
      const int64_t most = holds < limit ? holds : limit;
      if (wire_call)
        return fail(WEKWS_HIP_EINVAL, "%s: row %d: %d samples of %d bytes (%s) outside 0..%lld: row_bytes is %d", what, bad,
                    nsamp ? nsamp[bad] : int(holds), bp.wire_bytes[size_t(members[bad])], wire_name(bp.wire[size_t(members[bad])]),
                    (long long)most, width);
      return fail(WEKWS_HIP_EINVAL, "%s: row %d: %d samples outside 0..%lld", what, bad, nsamp ? nsamp[bad] : width, (long long)most);
    }
  }
  return WEKWS_HIP_OK;
}

// a refused push (resample_streams.h: resample_streams_plan), in words
int fail_push(const Rs* o, wekws::ResampleStreamsRefusal r, int bad, const char* what, int wire_call, const void* pcm, int width,
              const int32_t* ids, const int32_t* nsamp, int mcap) {
  const wekws::ResampleStreams& S = o->streams;
  switch (r) {
    case wekws::kResampleStreamsOk: break;
    case wekws::kResampleStreamsId:
      return fail(WEKWS_HIP_EINVAL, "%s: row %d: stream %d outside 0..%d", what, bad, ids[bad], S.max_streams - 1);
    case wekws::kResampleStreamsTwice:
      return fail(WEKWS_HIP_EINVAL, "%s: row %d: stream %d is given twice", what, bad, ids[bad]);
    case wekws::kResampleStreamsRows:
      return fail_rows(o->bank, S.rows, bad, what, wire_call, pcm, width, nsamp, S.members_of.data(), S.max_chunk);
    case wekws::kResampleStreamsFlushed:
      return fail(WEKWS_HIP_EINVAL, "%s: row %d: stream %d was flushed; reset it first", what, bad, ids[bad]);
    case wekws::kResampleStreamsInternal:
      return fail(WEKWS_HIP_EINVAL, "%s: internal: plan outside the handle's buffers", what);
    case wekws::kResampleStreamsCap:
      return fail(WEKWS_HIP_EINVAL, "%s: a row yields %lld samples, mcap is %d", what, (long long)S.need_cap, mcap);
  }
  return WEKWS_HIP_OK;
}

// The next slot of the table ring, free and large enough for B rows.  Calls queue back to back without a synchronise: the host
// waits only for the call that used the slot kResampleRing calls ago; a slot too small is replaced behind that wait (so no launch
// still reads it).
int take_slot(Rs* o, int B, hipStream_t s, const char* what, Rs::Slot** out) {
  Rs::Slot& slot = o->ring[o->next];
  if (slot.used) {
    const hipError_t e = hipEventSynchronize(slot.ev);
    if (e != hipSuccess) return hip_fail_at(e, what, ": table ring");
    slot.used = false;
  }
  if (size_t(B) > slot.cap) {
    if (stream_is_capturing(s)) return fail(WEKWS_HIP_EINVAL, "%s: %d rows need a larger table: not inside a capture", what, B);
    if (slot.h) (void)hipHostFree(slot.h);
    if (slot.d) (void)hipFree(slot.d);
    slot.h = nullptr; slot.d = nullptr; slot.cap = 0;
    HIP_TRY(hipHostMalloc(&slot.h, size_t(B) * sizeof(wekws::ResampleRow), hipHostMallocDefault));
    HIP_TRY(hipMalloc(&slot.d, size_t(B) * sizeof(wekws::ResampleRow)));
    if (!slot.ev) HIP_TRY(hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming));
    slot.cap = size_t(B);
  }
  o->next = (o->next + 1) % wekws::kResampleRing;
  *out = &slot;
  return WEKWS_HIP_OK;
}

// The slot's table (in slot order) goes to the device and the handle's kernel is launched over it.  *launched: the launch was
// issued, so a push has moved its streams' history.
int upload_and_launch(Rs* o, Rs::Slot& slot, int source, const void* pcm, int width, int16_t* hist, void* out, int B, int mcap,
                      hipStream_t s, const char* what, bool* launched) {
  *launched = false;
  hipError_t e = hipMemcpyAsync(slot.d, slot.h, size_t(B) * sizeof(wekws::ResampleRow), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_fail_at(e, what, ": table upload");
  *launched = true;
  const int rc = o->kind == Rs::kSingle
      ? wekws::launch_resample(o->P[0], o->lds, source == wekws::kResampleBankI16, o->out_i16, slot.d, pcm, width, hist, out, B, mcap,
                               o->max_grid, s)
      : wekws::launch_resample_bank(o->d_params, o->lds, source, o->out_i16, slot.d, pcm, width, hist, out, B, mcap, o->max_grid, s);
  e = hipEventRecord(slot.ev, s);
  slot.used = e == hipSuccess;
  if (rc) return hip_fail_at(hipGetLastError(), what, " launch");
  if (e != hipSuccess) return hip_fail_at(e, what, ": event");
  return WEKWS_HIP_OK;
}

}  // namespace

namespace wekws {

void resample_destroy(void* h) {
  Rs* o = static_cast<Rs*>(h);
  if (!o) return;
  DeviceGuard g(o->device);
  (void)hipDeviceSynchronize();
  for (Rs::Slot& t : o->ring) {
    if (t.ev) (void)hipEventDestroy(t.ev);
    if (t.h) (void)hipHostFree(t.h);
    if (t.d) (void)hipFree(t.d);
  }
  for (float* p : o->d_live) if (p) (void)hipFree(p);
  for (float* p : o->d_full) if (p) (void)hipFree(p);
  for (int32_t* p : o->d_meta) if (p) (void)hipFree(p);
  if (o->d_params) (void)hipFree(o->d_params);
  if (o->hist) (void)hipFree(o->hist);
  delete o;
}

int resample_create(int kind, const wekws_hip_resample_cfg* cfg, const int32_t* rates, const int32_t* encs, int num, void** out) {
  if (!cfg || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  ResampleBankPlan bank;
  if (int rc = plan_cfg(kind, cfg, rates, encs, num, &bank)) return rc;
  const int hist_cap = resample_bank_hist_cap(bank);
  if (int64_t(cfg->max_streams) * 2 * hist_cap > 0x7fffffffLL || int64_t(cfg->max_chunk) > 0x3fffffffLL)
    return fail(WEKWS_HIP_EINVAL, "%s: max_streams %d x max_chunk %d is out of range", kind == Rs::kSingle ? "resample" : "resample_bank",
                cfg->max_streams, cfg->max_chunk);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev)
    return fail(WEKWS_HIP_EDEVICE, "device %d of %d", cfg->device, ndev);
  Rs* o = new (std::nothrow) Rs;
  if (!o) return fail(WEKWS_HIP_ENOMEM, "host allocation failed");
  const size_t M = size_t(num), ns = size_t(cfg->max_streams);
  o->kind = kind;
  o->device = cfg->device;
  o->out_i16 = cfg->out_dtype == WEKWS_HIP_RESAMPLE_OUT_I16;
  o->lds = size_t(resample_bank_lds_bytes(bank));
  o->P.assign(M, ResampleParams{});
  o->d_live.assign(M, nullptr); o->d_full.assign(M, nullptr); o->d_meta.assign(M, nullptr);
  resample_streams_init(&o->streams, cfg->max_streams, cfg->max_chunk, hist_cap, kind == Rs::kSingle);
  DeviceGuard g(cfg->device);
  hipError_t e = hipSuccess;
  for (size_t k = 0; k < M && e == hipSuccess; ++k) {
    ResamplePlan& plan = bank.members[k];
    resample_plan_taps(&plan);
    const int n = plan.n, K = plan.K, stride = resample_stride(plan.max_live);
    std::vector<float> live(size_t(n) * stride, 0.f);
    std::vector<int32_t> meta(size_t(2) * n);
    for (int i = 0; i < n; ++i) {
      const int first = plan.first[size_t(i)], last = plan.last[size_t(i)];
      meta[size_t(i)] = first;
      meta[size_t(n) + i] = last - first + 1;
      for (int m = first; m <= last; ++m) live[size_t(i) * stride + (m - first)] = plan.taps[size_t(i) * K + m];
    }
    e = hipMalloc(&o->d_live[k], live.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(o->d_live[k], live.data(), live.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&o->d_full[k], plan.taps.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(o->d_full[k], plan.taps.data(), plan.taps.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&o->d_meta[k], meta.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(o->d_meta[k], meta.data(), meta.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    int64_t tile_off = 0;
    (void)resample_lds_bytes(plan, &tile_off);
    ResampleParams& P = o->P[k];
    P.o = plan.o; P.n = n; P.K = K; P.width = plan.width;
    P.stride = stride;
    P.tile_cap = int32_t(resample_tile_cap(plan));
    P.tile_off = int32_t(tile_off);
    P.live = o->d_live[k]; P.first = o->d_meta[k]; P.count = o->d_meta[k] + n; P.full = o->d_full[k];
  }
  if (e == hipSuccess) e = hipMalloc(&o->d_params, M * sizeof(ResampleParams));
  if (e == hipSuccess) e = hipMemcpy(o->d_params, o->P.data(), M * sizeof(ResampleParams), hipMemcpyHostToDevice);
  if (e == hipSuccess && ns > 0) e = hipMalloc(&o->hist, ns * 2 * size_t(hist_cap) * sizeof(int16_t));
  if (e == hipSuccess && ns > 0) e = hipMemset(o->hist, 0, ns * 2 * size_t(hist_cap) * sizeof(int16_t));
  // a push never has more rows than streams: its tables are allocated here, once
  for (int i = 0; i < kResampleRing && e == hipSuccess && ns > 0; ++i) {
    Rs::Slot& t = o->ring[i];
    e = hipHostMalloc(&t.h, ns * sizeof(ResampleRow), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&t.d, ns * sizeof(ResampleRow));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t.ev, hipEventDisableTiming);
    if (e == hipSuccess) t.cap = ns;
  }
  hipDeviceProp_t prop;
  if (e == hipSuccess) e = hipGetDeviceProperties(&prop, cfg->device);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = hip_fail_at(e, o->name(), " create");
    resample_destroy(o);
    return rc;
  }
  o->default_grid = o->max_grid = prop.multiProcessorCount > 0 ? prop.multiProcessorCount * 8 : 2048;
  o->bank = std::move(bank);
  *out = o;
  return WEKWS_HIP_OK;
}

int resample_max_out(void* h, int nmax, int flush) {
  Rs* o = static_cast<Rs*>(h);
  if (!o || nmax < 0) return 0;
  const int64_t m = resample_bank_max_out(o->bank, nmax, flush);
  return int(m > 0x7fffffffLL ? 0x7fffffffLL : m);
}

// one-shot: row b an utterance of nsamp[b] samples (NULL: as many as the row holds) at member member_of_row[b]'s rate, from its first
// sample (source: ResampleBankSource; width: the row's width in samples, or in bytes for wire rows)
int resample_compute(void* h, int source, const void* pcm, int B, int width, const int32_t* nsamp, const int32_t* member_of_row, void* out,
                     int mcap, void* stream_) {
  Rs* o = static_cast<Rs*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  const int wire_call = source == kResampleBankWireBytes;
  const char* const what = kEntry[o->kind][0][wire_call];
  if (B < 0 || width < 0 || mcap < 0 || width > 0x3fffffff || mcap > 0x3fffffff)
    return fail(WEKWS_HIP_EINVAL, "%s: B=%d %s=%d mcap=%d", what, B, wire_call ? "row_bytes" : "nmax", width, mcap);
  if (B == 0) return WEKWS_HIP_OK;
  if (!member_of_row && o->kind != Rs::kSingle) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(o->mu);
  const ResampleBankPlan& bp = o->bank;
  if (!member_of_row) {
    o->streams.members_of.assign(size_t(B), 0);
    member_of_row = o->streams.members_of.data();
  }
  // ---- the rows are checked before anything else: a refusal launches nothing
  const int64_t limit = 0x3fffffff;
  int bad = -1;
  const ResampleBankRowRefusal r =
      resample_bank_check_rows(bp, wire_call, uint64_t(reinterpret_cast<uintptr_t>(pcm)), width, nsamp, member_of_row, B, limit, &bad);
  if (r != kResampleRowsOk) return fail_rows(bp, r, bad, what, wire_call, pcm, width, nsamp, member_of_row, limit);
  auto len_of = [&](int b) { return nsamp ? nsamp[b] : int32_t(resample_bank_row_samples(bp, wire_call, member_of_row[b], width)); };
  for (int b = 0; b < B; ++b) {
    const int64_t cnt = resample_once_count(bp, member_of_row[b], len_of(b));
    if (cnt > mcap) return fail(WEKWS_HIP_EINVAL, "%s: row %d yields %lld samples, mcap is %d", what, b, (long long)cnt, mcap);
  }
  if (mcap == 0) return WEKWS_HIP_OK;            // (no row yields a sample: checked above)
  if (!out || (width > 0 && !pcm)) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream_);
  Rs::Slot* slot = nullptr;
  if (int rc = take_slot(o, B, s, what, &slot)) return rc;
  const int32_t* pos = resample_slot_positions(&o->streams, member_of_row, B, int(bp.members.size()));
  for (int b = 0; b < B; ++b) resample_once_row(bp, wire_call, member_of_row[b], b, len_of(b), &slot->h[pos ? pos[b] : b]);
  bool launched;
  return upload_and_launch(o, *slot, source, pcm, width, nullptr, out, B, mcap, s, what, &launched);
}

// (wire_call: pcm is (B, width) BYTES in the encodings of the rows' members; otherwise (B, width) int16)
int resample_push(void* h, int wire_call, const void* pcm, int B, int width, const int32_t* stream_ids, const int32_t* nsamp, int flush,
                  void* out, int mcap, int32_t* counts, void* stream_) {
  Rs* o = static_cast<Rs*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  const char* const what = kEntry[o->kind][1][wire_call];
  ResampleStreams& S = o->streams;
  if (B < 0 || width < 0 || mcap < 0) return fail(WEKWS_HIP_EINVAL, "%s: B=%d %s=%d mcap=%d", what, B, wire_call ? "row_bytes" : "nmax", width, mcap);
  if (B == 0) return WEKWS_HIP_OK;
  if (!stream_ids || !nsamp || !counts || (width > 0 && !pcm)) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (S.max_streams < 1) return fail(WEKWS_HIP_EINVAL, "%s: the handle was created without streams (max_streams 0)", what);
  if (!wire_call && width > S.max_chunk) return fail(WEKWS_HIP_EINVAL, "%s: nmax %d > max_chunk %d", what, width, S.max_chunk);
  if (B > S.max_streams) return fail(WEKWS_HIP_EINVAL, "%s: %d rows for %d streams", what, B, S.max_streams);
  if (int64_t(B) * mcap > (int64_t(1) << 40)) return fail(WEKWS_HIP_EINVAL, "%s: B %d x mcap %d is out of range", what, B, mcap);
  std::lock_guard<std::mutex> lk(o->mu);
  // ---- the whole call is planned first: a refusal launches nothing and changes no stream
  int bad = -1;
  const ResampleStreamsRefusal r =
      resample_streams_plan(&S, o->bank, wire_call, uint64_t(reinterpret_cast<uintptr_t>(pcm)), width, stream_ids, nsamp, B, flush, mcap, &bad);
  if (r != kResampleStreamsOk) return fail_push(o, r, bad, what, wire_call, pcm, width, stream_ids, nsamp, mcap);
  if (mcap > 0 && !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream_);
  Rs::Slot* slot = nullptr;
  if (int rc = take_slot(o, B, s, what, &slot)) return rc;
  // ---- every row straight into its place in the pinned table
  const int32_t* pos = resample_slot_positions(&S, S.members_of.data(), B, int(o->bank.members.size()));
  resample_streams_push_rows(S, o->bank, wire_call, stream_ids, nsamp, B, pos, slot->h);
  // ---- one launch; from there the streams' state moves
  bool launched;
  const int rc = upload_and_launch(o, *slot, wire_call ? kResampleBankWireBytes : kResampleBankI16, pcm, width, o->hist, out, B, mcap, s,
                                   what, &launched);
  if (launched) resample_streams_commit(&S, stream_ids, nsamp, B, flush, counts);
  return rc;
}

int resample_reset(void* h, const int32_t* ids, int n, const int* member) {
  Rs* o = static_cast<Rs*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  const char* const entry = member ? "set_rate" : "reset";
  if (n < 0 || (n > 0 && !ids)) return fail(WEKWS_HIP_EINVAL, "%s_%s: n=%d", o->name(), entry, n);
  const int M = int(o->bank.members.size());
  if (member && (*member < 0 || *member >= M))
    return fail(WEKWS_HIP_EINVAL, "%s_%s: member %d outside 0..%d", o->name(), entry, *member, M - 1);
  std::lock_guard<std::mutex> lk(o->mu);
  const int bad = resample_streams_reset(&o->streams, ids, n, member ? *member : -1);
  if (bad >= 0) return fail(WEKWS_HIP_EINVAL, "%s_%s: stream %d outside 0..%d", o->name(), entry, ids[bad], o->streams.max_streams - 1);
  return WEKWS_HIP_OK;
}

int resample_counts(void* h, int id, int64_t counts_out[4]) {
  Rs* o = static_cast<Rs*>(h);
  if (!o || !counts_out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (id < 0 || id >= o->streams.max_streams)
    return fail(WEKWS_HIP_EINVAL, "%s_counts: stream %d outside 0..%d", o->name(), id, o->streams.max_streams - 1);
  std::lock_guard<std::mutex> lk(o->mu);
  resample_streams_counts(o->streams, id, counts_out);
  return WEKWS_HIP_OK;
}

}  // namespace wekws

// ------------------------------------------------------------------------------------------------ C ABI of the rate bank
extern "C" {

int wekws_hip_wire_sample_bytes(int encoding) { return wekws::wire_sample_bytes(encoding); }

int wekws_hip_wire_decode(int encoding, const void* src, int64_t n, int16_t* dst) {
  const int bytes = wekws::wire_sample_bytes(encoding);
  if (!bytes) return fail(WEKWS_HIP_EINVAL, "wire_decode: encoding %d is none of s16, mulaw, alaw, u8, f32", encoding);
  if (n < 0 || (n > 0 && (!src || !dst))) return fail(WEKWS_HIP_EINVAL, "wire_decode: n=%lld or a NULL pointer", (long long)n);
  const uint8_t* p = static_cast<const uint8_t*>(src);
  for (int64_t k = 0; k < n; ++k) {
    if (bytes == 1) {
      dst[k] = int16_t(wekws::wire_byte(encoding, p[k]));
    } else if (bytes == 2) {
      dst[k] = int16_t(uint16_t(p[2 * k] | (p[2 * k + 1] << 8)));
    } else {
      const uint32_t u = uint32_t(p[4 * k]) | (uint32_t(p[4 * k + 1]) << 8) | (uint32_t(p[4 * k + 2]) << 16) | (uint32_t(p[4 * k + 3]) << 24);
      float x;
      std::memcpy(&x, &u, 4);
      dst[k] = int16_t(wekws::wire_f32(x));
    }
  }
  return WEKWS_HIP_OK;
}

int wekws_hip_resample_bank_create(const wekws_hip_resample_cfg* cfg, const int32_t* orig_freqs, int num_rates, void** out) {
  return wekws::resample_create(Rs::kBank, cfg, orig_freqs, nullptr, num_rates, out);
}

int wekws_hip_resample_bank_create_wire(const wekws_hip_resample_cfg* cfg, const int32_t* orig_freqs, const int32_t* encodings,
                                        int num_rates, void** out) {
  if (!encodings) {
    if (out) *out = nullptr;
    return fail(WEKWS_HIP_EINVAL, "NULL argument");
  }
  return wekws::resample_create(Rs::kBank, cfg, orig_freqs, encodings, num_rates, out);
}

void wekws_hip_resample_bank_destroy(void* h) { wekws::resample_destroy(h); }

int wekws_hip_resample_bank_max_out(void* h, int nmax, int flush) { return wekws::resample_max_out(h, nmax, flush); }

int wekws_hip_resample_bank_compute(void* h, const float* pcm, int B, int nmax, const int32_t* nsamp, const int32_t* member_of_row,
                                    void* out, int mcap, void* stream) {
  return wekws::resample_compute(h, wekws::kResampleBankF32, pcm, B, nmax, nsamp, member_of_row, out, mcap, stream);
}

int wekws_hip_resample_bank_compute_i16(void* h, const int16_t* pcm, int B, int nmax, const int32_t* nsamp,
                                        const int32_t* member_of_row, void* out, int mcap, void* stream) {
  return wekws::resample_compute(h, wekws::kResampleBankI16, pcm, B, nmax, nsamp, member_of_row, out, mcap, stream);
}

int wekws_hip_resample_bank_compute_wire(void* h, const uint8_t* pcm, int B, int row_bytes, const int32_t* nsamp,
                                         const int32_t* member_of_row, void* out, int mcap, void* stream) {
  return wekws::resample_compute(h, wekws::kResampleBankWireBytes, pcm, B, row_bytes, nsamp, member_of_row, out, mcap, stream);
}

int wekws_hip_resample_bank_push(void* h, const int16_t* pcm, int B, int nmax, const int32_t* stream_ids, const int32_t* nsamp,
                                 int flush, void* out, int mcap, int32_t* counts, void* stream) {
  return wekws::resample_push(h, 0, pcm, B, nmax, stream_ids, nsamp, flush, out, mcap, counts, stream);
}

int wekws_hip_resample_bank_push_wire(void* h, const uint8_t* pcm, int B, int row_bytes, const int32_t* stream_ids,
                                      const int32_t* nsamp, int flush, void* out, int mcap, int32_t* counts, void* stream) {
  return wekws::resample_push(h, 1, pcm, B, row_bytes, stream_ids, nsamp, flush, out, mcap, counts, stream);
}

int wekws_hip_resample_bank_set_rate(void* h, const int32_t* ids, int n, int member) { return wekws::resample_reset(h, ids, n, &member); }

int wekws_hip_resample_bank_reset(void* h, const int32_t* ids, int n) { return wekws::resample_reset(h, ids, n, nullptr); }

int wekws_hip_resample_bank_counts(void* h, int id, int64_t counts_out[4]) { return wekws::resample_counts(h, id, counts_out); }

int wekws_hip_resample_bank_rate_of(void* h, int id) {
  Rs* o = static_cast<Rs*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (id < 0 || id >= o->streams.max_streams)
    return fail(WEKWS_HIP_EINVAL, "resample_bank_rate_of: stream %d outside 0..%d", id, o->streams.max_streams - 1);
  std::lock_guard<std::mutex> lk(o->mu);
  return o->bank.members[size_t(o->streams.member[size_t(id)])].orig;
}

int wekws_hip_resample_bank_encoding_of(void* h, int id) {
  Rs* o = static_cast<Rs*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (id < 0 || id >= o->streams.max_streams)
    return fail(WEKWS_HIP_EINVAL, "resample_bank_encoding_of: stream %d outside 0..%d", id, o->streams.max_streams - 1);
  std::lock_guard<std::mutex> lk(o->mu);
  return o->bank.wire[size_t(o->streams.member[size_t(id)])];
}

}  // extern "C"
