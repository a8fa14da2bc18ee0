// Launcher, handle and C ABI of the rate bank (resample_bank.hip.h, resample_bank_plan.h).
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

// ------------------------------------------------------------------------------------------------ C ABI
namespace {

typedef wekws_hip_resample_bank Bank;

// the plan of a configuration, or the refusal: EINVAL for a bank or rates no resampler has, EUNSUPPORTED for a member whose live
// table does not fit the LDS budget
const char* wire_name(int enc) {
  static const char* const names[wekws::kWireCount] = {"s16", "mulaw", "alaw", "u8", "f32"};
  return enc >= 0 && enc < wekws::kWireCount ? names[enc] : "?";
}

// encs: NULL for wekws_hip_resample_bank_create (every member S16; a repeated rate is then the repeated pair)
int plan_bank(const wekws_hip_resample_cfg* c, const int32_t* rates, const int32_t* encs, int num, wekws::ResampleBankPlan* bp) {
  int bad = -1;
  const wekws::ResampleBankRefusal r =
      wekws::resample_bank_plan(rates, encs, num, c->new_freq, c->lowpass_filter_width, c->rolloff, bp, &bad);
  switch (r) {
    case wekws::kResampleBankOk: break;
    case wekws::kResampleBankWire:
      return fail(WEKWS_HIP_EINVAL, "resample_bank: member %d: encoding %d is none of s16, mulaw, alaw, u8, f32 (0..%d)", bad, encs[bad],
                  wekws::kWireCount - 1);
    case wekws::kResampleBankCount:
      return fail(WEKWS_HIP_EINVAL, "resample_bank: %d rates: a bank holds 1..%d", num, wekws::kResampleBankMax);
    case wekws::kResampleBankRate:
      return fail(WEKWS_HIP_EINVAL, "resample_bank: member %d: orig_freq %d, new_freq %d: rates are positive", bad,
                  bad >= 0 ? rates[bad] : 0, c->new_freq);
    case wekws::kResampleBankRepeat:
      if (encs) return fail(WEKWS_HIP_EINVAL, "resample_bank: member %d repeats the pair (%d, %s)", bad, rates[bad], wire_name(encs[bad]));
      return fail(WEKWS_HIP_EINVAL, "resample_bank: member %d repeats the rate %d", bad, rates[bad]);
    case wekws::kResampleBankParams:
      return fail(WEKWS_HIP_EINVAL, "resample_bank: lowpass_filter_width %d, rolloff %g (a width >= 1, 0 < rolloff <= 1)",
                  c->lowpass_filter_width, c->rolloff);
    case wekws::kResampleBankLds: {
      const wekws::ResamplePlan& p = bp->members[size_t(bad)];
      return fail(WEKWS_HIP_EUNSUPPORTED, "resample_bank: member %d, %d -> %d: %d phases x %d live taps and a tile of %lld samples need "
                  "%lld bytes of LDS, the budget is %d", bad, rates[bad], c->new_freq, p.n, p.max_live,
                  (long long)wekws::resample_tile_cap(p), (long long)wekws::resample_lds_bytes(p), wekws::kResampleLdsBudget);
    }
  }
  if (c->orig_freq != rates[0])
    return fail(WEKWS_HIP_EINVAL, "resample_bank: cfg.orig_freq %d is not member 0's rate %d", c->orig_freq, rates[0]);
  if (c->out_dtype != WEKWS_HIP_RESAMPLE_OUT_F32 && c->out_dtype != WEKWS_HIP_RESAMPLE_OUT_I16)
    return fail(WEKWS_HIP_EINVAL, "resample_bank: out_dtype %d", c->out_dtype);
  if (c->max_streams < 0 || (c->max_streams > 0 && c->max_chunk <= 0))
    return fail(WEKWS_HIP_EINVAL, "resample_bank: max_streams=%d max_chunk=%d", c->max_streams, c->max_chunk);
  return WEKWS_HIP_OK;
}

// The rows of a call (resample_bank_plan.h: resample_bank_check_rows), or the refusal in words.  width: nmax, or row_bytes of a
// wire call.
int check_rows(const Bank* o, const char* what, int wire_call, const void* pcm, int width, const int32_t* nsamp, const int32_t* members,
               int B, int64_t limit) {
  int bad = -1;
  const wekws::ResampleBankPlan& bp = o->bank;
  const wekws::ResampleBankRowRefusal r = wekws::resample_bank_check_rows(bp, wire_call, uint64_t(reinterpret_cast<uintptr_t>(pcm)), width,
                                                                          nsamp, members, B, limit, &bad);
  const int M = int(bp.members.size());
  switch (r) {
    case wekws::kResampleRowsOk: break;
    case wekws::kResampleRowsAlign:
      return fail(WEKWS_HIP_EINVAL, "%s: pcm %p is not %d-byte aligned", what, pcm, wekws::kResampleWireAlign);
    case wekws::kResampleRowsWidth:
      return fail(WEKWS_HIP_EINVAL, "%s: row_bytes %d: a multiple of %d in 0..2^30-4", what, width, wekws::kResampleWireAlign);
    case wekws::kResampleRowsMember:
      return fail(WEKWS_HIP_EINVAL, "%s: row %d: member %d outside 0..%d", what, bad, members[bad], M - 1);
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

// The next slot of the table ring, free and large enough for B rows.  Calls queue back to back without a synchronise: the host
// waits only for the call that used the slot kResampleRing calls ago; a slot too small is replaced behind that wait.
int take_slot(Bank* o, int B, hipStream_t s, const char* what, Bank::Slot** out) {
  Bank::Slot& slot = o->ring[o->next];
  if (slot.used) {
    const hipError_t e = hipEventSynchronize(slot.ev);
    if (e != hipSuccess) return hip_fail(e, what);
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

// o->table (row order, member and row filled in) goes to the slot in slot order -- sorted by member -- and is launched
int upload_and_launch(Bank* o, Bank::Slot& slot, int source, const void* pcm, int nmax, int16_t* hist, void* out, int B, int mcap,
                      hipStream_t s, const char* what) {
  o->order.resize(size_t(B));
  wekws::resample_bank_order(o->members_of.data(), B, int(o->rates.size()), o->order.data());
  for (int k = 0; k < B; ++k) slot.h[k] = o->table[size_t(o->order[size_t(k)])];
  hipError_t e = hipMemcpyAsync(slot.d, slot.h, size_t(B) * sizeof(wekws::ResampleRow), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_fail(e, what);
  const int rc = wekws::launch_resample_bank(o->d_params, o->lds, source, o->out_i16, slot.d, pcm, nmax, hist, out, B, mcap,
                                             o->max_grid, s);
  e = hipEventRecord(slot.ev, s);
  slot.used = e == hipSuccess;
  if (rc) return hip_fail(hipGetLastError(), what);
  if (e != hipSuccess) return hip_fail(e, what);
  return WEKWS_HIP_OK;
}

}  // namespace

extern "C" {

void wekws_hip_resample_bank_destroy(void* h) {
  Bank* o = static_cast<Bank*>(h);
  if (!o) return;
  DeviceGuard g(o->device);
  (void)hipDeviceSynchronize();
  for (Bank::Slot& t : o->ring) {
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

// encodings NULL: wekws_hip_resample_bank_create's bank, every member S16
static int create_bank(const wekws_hip_resample_cfg* cfg, const int32_t* orig_freqs, const int32_t* encodings, int num_rates, void** out) {
  if (!cfg || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  wekws::ResampleBankPlan bank;
  if (int rc = plan_bank(cfg, orig_freqs, encodings, num_rates, &bank)) return rc;
  const int hist_cap = wekws::resample_bank_hist_cap(bank);
  if (int64_t(cfg->max_streams) * 2 * hist_cap > 0x7fffffffLL || int64_t(cfg->max_chunk) > 0x3fffffffLL)
    return fail(WEKWS_HIP_EINVAL, "resample_bank: max_streams %d x max_chunk %d is out of range", cfg->max_streams, cfg->max_chunk);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev)
    return fail(WEKWS_HIP_EDEVICE, "device %d of %d", cfg->device, ndev);
  Bank* o = new (std::nothrow) Bank;
  if (!o) return fail(WEKWS_HIP_ENOMEM, "host allocation failed");
  const size_t M = size_t(num_rates), ns = size_t(cfg->max_streams);
  o->device = cfg->device;
  o->out_i16 = cfg->out_dtype == WEKWS_HIP_RESAMPLE_OUT_I16;
  o->max_streams = cfg->max_streams; o->max_chunk = cfg->max_chunk; o->hist_cap = hist_cap;
  o->rates.assign(orig_freqs, orig_freqs + num_rates);
  o->lds = size_t(wekws::resample_bank_lds_bytes(bank));
  o->P.assign(M, wekws::ResampleParams{});
  o->d_live.assign(M, nullptr); o->d_full.assign(M, nullptr); o->d_meta.assign(M, nullptr);
  o->received.assign(ns, 0); o->emitted.assign(ns, 0); o->origin.assign(ns, 0);
  o->par.assign(ns, 0); o->seen.assign(ns, 0); o->flushed.assign(ns, 0); o->member.assign(ns, 0);
  o->steps.reserve(ns);
  DeviceGuard g(cfg->device);
  hipError_t e = hipSuccess;
  for (size_t k = 0; k < M && e == hipSuccess; ++k) {
    wekws::ResamplePlan& plan = bank.members[k];
    wekws::resample_plan_taps(&plan);
    const int n = plan.n, K = plan.K, stride = wekws::resample_stride(plan.max_live);
    std::vector<float> live(size_t(n) * stride, 0.f);
    std::vector<int32_t> meta(size_t(2) * n);
    for (int i = 0; i < n; ++i) {
      meta[size_t(i)] = plan.first[size_t(i)];
      meta[size_t(n) + i] = plan.last[size_t(i)] - plan.first[size_t(i)] + 1;
      for (int m = plan.first[size_t(i)]; m <= plan.last[size_t(i)]; ++m)
        live[size_t(i) * stride + (m - plan.first[size_t(i)])] = plan.taps[size_t(i) * K + m];
    }
    e = hipMalloc(&o->d_live[k], live.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(o->d_live[k], live.data(), live.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&o->d_full[k], plan.taps.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(o->d_full[k], plan.taps.data(), plan.taps.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&o->d_meta[k], meta.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(o->d_meta[k], meta.data(), meta.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    int64_t tile_off = 0;
    (void)wekws::resample_lds_bytes(plan, &tile_off);
    wekws::ResampleParams& P = o->P[k];
    P.o = plan.o; P.n = n; P.K = K; P.width = plan.width;
    P.stride = stride;
    P.tile_cap = int32_t(wekws::resample_tile_cap(plan));
    P.tile_off = int32_t(tile_off);
    P.live = o->d_live[k]; P.first = o->d_meta[k]; P.count = o->d_meta[k] + n; P.full = o->d_full[k];
  }
  if (e == hipSuccess) e = hipMalloc(&o->d_params, M * sizeof(wekws::ResampleParams));
  if (e == hipSuccess) e = hipMemcpy(o->d_params, o->P.data(), M * sizeof(wekws::ResampleParams), hipMemcpyHostToDevice);
  if (e == hipSuccess && ns > 0) e = hipMalloc(&o->hist, ns * 2 * size_t(hist_cap) * sizeof(int16_t));
  if (e == hipSuccess && ns > 0) e = hipMemset(o->hist, 0, ns * 2 * size_t(hist_cap) * sizeof(int16_t));
  // a push never has more rows than streams: its tables are allocated here, once
  for (int i = 0; i < wekws::kResampleRing && e == hipSuccess && ns > 0; ++i) {
    Bank::Slot& t = o->ring[i];
    e = hipHostMalloc(&t.h, ns * sizeof(wekws::ResampleRow), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&t.d, ns * sizeof(wekws::ResampleRow));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t.ev, hipEventDisableTiming);
    if (e == hipSuccess) t.cap = ns;
  }
  hipDeviceProp_t prop;
  if (e == hipSuccess) e = hipGetDeviceProperties(&prop, cfg->device);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = hip_fail(e, "resample_bank create");
    wekws_hip_resample_bank_destroy(o);
    return rc;
  }
  o->default_grid = o->max_grid = prop.multiProcessorCount > 0 ? prop.multiProcessorCount * 8 : 2048;
  o->bank = std::move(bank);
  *out = o;
  return WEKWS_HIP_OK;
}

int wekws_hip_resample_bank_create(const wekws_hip_resample_cfg* cfg, const int32_t* orig_freqs, int num_rates, void** out) {
  return create_bank(cfg, orig_freqs, nullptr, num_rates, out);
}

int wekws_hip_resample_bank_create_wire(const wekws_hip_resample_cfg* cfg, const int32_t* orig_freqs, const int32_t* encodings,
                                        int num_rates, void** out) {
  if (!encodings) {
    if (out) *out = nullptr;
    return fail(WEKWS_HIP_EINVAL, "NULL argument");
  }
  return create_bank(cfg, orig_freqs, encodings, num_rates, out);
}

int wekws_hip_resample_bank_max_out(void* h, int nmax, int flush) {
  Bank* o = static_cast<Bank*>(h);
  if (!o || nmax < 0) return 0;
  const int64_t m = wekws::resample_bank_max_out(o->bank, nmax, flush);
  return int(m > 0x7fffffffLL ? 0x7fffffffLL : m);
}

}  // extern "C"

namespace {

// one-shot: row b an utterance of nsamp[b] samples (NULL: nmax) at member member_of_row[b]'s rate, from its first sample
// (source: wekws::ResampleBankSource; nmax: the row's width in samples, or in bytes for wire rows)
int compute(void* h, const void* pcm, int source, int B, int nmax, const int32_t* nsamp, const int32_t* member_of_row, void* out,
            int mcap, void* stream_) {
  Bank* o = static_cast<Bank*>(h);
  const int wire_call = source == wekws::kResampleBankWireBytes;
  const char* const what = wire_call ? "resample_bank_compute_wire" : "resample_bank_compute";
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (B < 0 || nmax < 0 || mcap < 0 || nmax > 0x3fffffff || mcap > 0x3fffffff)
    return fail(WEKWS_HIP_EINVAL, "%s: B=%d %s=%d mcap=%d", what, B, wire_call ? "row_bytes" : "nmax", nmax, mcap);
  if (B == 0) return WEKWS_HIP_OK;
  if (!member_of_row) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(o->mu);
  if (int rc = check_rows(o, what, wire_call, pcm, nmax, nsamp, member_of_row, B, 0x3fffffff)) return rc;
  o->table.clear();
  o->members_of.assign(member_of_row, member_of_row + B);
  for (int b = 0; b < B; ++b) {
    const int m = member_of_row[b];
    const int len = nsamp ? nsamp[b] : int(wekws::resample_bank_row_samples(o->bank, wire_call, m, nmax));
    const wekws::ResamplePlan& p = o->bank.members[size_t(m)];
    const int64_t cnt = wekws::resample_num_samples(p, len);
    if (cnt > mcap) return fail(WEKWS_HIP_EINVAL, "%s: row %d yields %lld samples, mcap is %d", what, b, (long long)cnt, mcap);
    wekws::ResampleRow R{};
    R.i0 = 0; R.base_rel = -p.width; R.cnt = int32_t(cnt); R.h = 0; R.hi_valid = len;
    R.member = m; R.row = b;
    R.wire = wire_call ? o->bank.wire[size_t(m)] : 0;
    o->table.push_back(R);
  }
  if (mcap == 0) return WEKWS_HIP_OK;            // (no row yields a sample: checked above)
  if (!out || (nmax > 0 && !pcm)) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream_);
  Bank::Slot* slot = nullptr;
  if (int rc = take_slot(o, B, s, "resample_bank_compute: table ring", &slot)) return rc;
  return upload_and_launch(o, *slot, source, pcm, nmax, nullptr, out, B, mcap, s, "resample_bank_compute launch");
}

}  // namespace

extern "C" {

int wekws_hip_resample_bank_compute(void* h, const float* pcm, int B, int nmax, const int32_t* nsamp, const int32_t* member_of_row,
                                    void* out, int mcap, void* stream) {
  return compute(h, pcm, wekws::kResampleBankF32, B, nmax, nsamp, member_of_row, out, mcap, stream);
}

int wekws_hip_resample_bank_compute_i16(void* h, const int16_t* pcm, int B, int nmax, const int32_t* nsamp,
                                        const int32_t* member_of_row, void* out, int mcap, void* stream) {
  return compute(h, pcm, wekws::kResampleBankI16, B, nmax, nsamp, member_of_row, out, mcap, stream);
}

int wekws_hip_resample_bank_compute_wire(void* h, const uint8_t* pcm, int B, int row_bytes, const int32_t* nsamp,
                                         const int32_t* member_of_row, void* out, int mcap, void* stream) {
  return compute(h, pcm, wekws::kResampleBankWireBytes, B, row_bytes, nsamp, member_of_row, out, mcap, stream);
}

// (wire_call: pcm is (B, nmax) BYTES in the encodings of the rows' members; otherwise (B, nmax) int16)
static int push(void* h, const void* pcm, int wire_call, int B, int nmax, const int32_t* stream_ids, const int32_t* nsamp, int flush,
                void* out, int mcap, int32_t* counts, void* stream_) {
  Bank* o = static_cast<Bank*>(h);
  const char* const what = wire_call ? "resample_bank_push_wire" : "resample_bank_push";
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (B < 0 || nmax < 0 || mcap < 0) return fail(WEKWS_HIP_EINVAL, "%s: B=%d %s=%d mcap=%d", what, B, wire_call ? "row_bytes" : "nmax", nmax, mcap);
  if (B == 0) return WEKWS_HIP_OK;
  if (!stream_ids || !nsamp || !counts || (nmax > 0 && !pcm)) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (o->max_streams < 1) return fail(WEKWS_HIP_EINVAL, "%s: the handle was created without streams (max_streams 0)", what);
  if (!wire_call && nmax > o->max_chunk) return fail(WEKWS_HIP_EINVAL, "%s: nmax %d > max_chunk %d", what, nmax, o->max_chunk);
  if (B > o->max_streams) return fail(WEKWS_HIP_EINVAL, "%s: %d rows for %d streams", what, B, o->max_streams);
  if (int64_t(B) * mcap > (int64_t(1) << 40)) return fail(WEKWS_HIP_EINVAL, "%s: B %d x mcap %d is out of range", what, B, mcap);
  std::lock_guard<std::mutex> lk(o->mu);
  // ---- the whole call is planned first: a refusal launches nothing and changes no stream.  (epoch / seen are scratch of this
  // planning pass and carry nothing from one call to the next: a refused call may leave them advanced.)
  if (++o->epoch == 0x7fffffff) { o->epoch = 1; o->seen.assign(o->seen.size(), 0); }
  o->steps.clear();
  o->members_of.resize(size_t(B));
  for (int b = 0; b < B; ++b) {
    const int id = stream_ids[b];
    if (id < 0 || id >= o->max_streams) return fail(WEKWS_HIP_EINVAL, "%s: row %d: stream %d outside 0..%d", what, b, id, o->max_streams - 1);
    if (o->seen[id] == o->epoch) return fail(WEKWS_HIP_EINVAL, "%s: row %d: stream %d is given twice", what, b, id);
    o->seen[id] = o->epoch;
    o->members_of[size_t(b)] = o->member[id];
  }
  // the rows as their streams' members read them: lengths in samples against max_chunk and against the bytes of the row
  if (int rc = check_rows(o, what, wire_call, pcm, nmax, nsamp, o->members_of.data(), B, o->max_chunk)) return rc;
  int64_t need_cap = 0;
  for (int b = 0; b < B; ++b) {
    const int id = stream_ids[b];
    if (o->flushed[id]) return fail(WEKWS_HIP_EINVAL, "%s: row %d: stream %d was flushed; reset it first", what, b, id);
    const wekws::ResampleStep st = wekws::resample_step(o->bank.members[size_t(o->member[id])], o->received[id], nsamp[b], flush);
    const int64_t N2 = o->received[id] + nsamp[b];
    if (N2 - st.keep_from > o->hist_cap || st.keep_from < o->origin[id] || st.total < o->emitted[id])
      return fail(WEKWS_HIP_EINVAL, "%s: internal: plan outside the handle's buffers", what);
    if (st.total - o->emitted[id] > need_cap) need_cap = st.total - o->emitted[id];
    o->steps.push_back(st);
  }
  if (need_cap > mcap) return fail(WEKWS_HIP_EINVAL, "%s: a row yields %lld samples, mcap is %d", what, (long long)need_cap, mcap);
  if (mcap > 0 && !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream_);
  Bank::Slot* slot = nullptr;
  if (int rc = take_slot(o, B, s, "resample_bank_push: plan ring", &slot)) return rc;
  o->table.resize(size_t(B));
  o->members_of.resize(size_t(B));
  for (int b = 0; b < B; ++b) {
    const int id = stream_ids[b], m = o->member[id];
    const wekws::ResamplePlan& p = o->bank.members[size_t(m)];
    const wekws::ResampleStep& st = o->steps[size_t(b)];
    const int64_t q0 = o->emitted[id], j0 = q0 / p.n, s0 = o->origin[id];
    wekws::ResampleRow& R = o->table[size_t(b)];
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
    R.member = m; R.row = b;
    R.wire = wire_call ? o->bank.wire[size_t(m)] : 0;
    o->members_of[size_t(b)] = m;
  }
  // ---- one launch; from here the streams' state moves
  const int rc = upload_and_launch(o, *slot, wire_call ? wekws::kResampleBankWireBytes : wekws::kResampleBankI16, pcm, nmax, o->hist, out, B,
                                   mcap, s, "resample_bank_push launch");
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
  return rc;
}

int wekws_hip_resample_bank_push(void* h, const int16_t* pcm, int B, int nmax, const int32_t* stream_ids, const int32_t* nsamp,
                                 int flush, void* out, int mcap, int32_t* counts, void* stream) {
  return push(h, pcm, 0, B, nmax, stream_ids, nsamp, flush, out, mcap, counts, stream);
}

int wekws_hip_resample_bank_push_wire(void* h, const uint8_t* pcm, int B, int row_bytes, const int32_t* stream_ids,
                                      const int32_t* nsamp, int flush, void* out, int mcap, int32_t* counts, void* stream) {
  return push(h, pcm, 1, B, row_bytes, stream_ids, nsamp, flush, out, mcap, counts, stream);
}

int wekws_hip_resample_bank_encoding_of(void* h, int id) {
  Bank* o = static_cast<Bank*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (id < 0 || id >= o->max_streams) return fail(WEKWS_HIP_EINVAL, "resample_bank_encoding_of: stream %d outside 0..%d", id, o->max_streams - 1);
  std::lock_guard<std::mutex> lk(o->mu);
  return o->bank.wire[size_t(o->member[id])];
}

int wekws_hip_resample_bank_set_rate(void* h, const int32_t* ids, int n, int member) {
  Bank* o = static_cast<Bank*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (n < 0 || (n > 0 && !ids)) return fail(WEKWS_HIP_EINVAL, "resample_bank_set_rate: n=%d", n);
  if (member < 0 || member >= int(o->rates.size()))
    return fail(WEKWS_HIP_EINVAL, "resample_bank_set_rate: member %d outside 0..%d", member, int(o->rates.size()) - 1);
  std::lock_guard<std::mutex> lk(o->mu);
  for (int i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= o->max_streams)
      return fail(WEKWS_HIP_EINVAL, "resample_bank_set_rate: stream %d outside 0..%d", ids[i], o->max_streams - 1);
  // the counts ARE the state: a stream that has received nothing reads nothing of its device buffers
  for (int i = 0; i < n; ++i) {
    const int id = ids[i];
    o->member[id] = member;
    o->received[id] = 0; o->emitted[id] = 0; o->origin[id] = 0; o->flushed[id] = 0;
  }
  return WEKWS_HIP_OK;
}

int wekws_hip_resample_bank_rate_of(void* h, int id) {
  Bank* o = static_cast<Bank*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (id < 0 || id >= o->max_streams) return fail(WEKWS_HIP_EINVAL, "resample_bank_rate_of: stream %d outside 0..%d", id, o->max_streams - 1);
  std::lock_guard<std::mutex> lk(o->mu);
  return o->rates[size_t(o->member[id])];
}

int wekws_hip_resample_bank_reset(void* h, const int32_t* ids, int n) {
  Bank* o = static_cast<Bank*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (n < 0 || (n > 0 && !ids)) return fail(WEKWS_HIP_EINVAL, "resample_bank_reset: n=%d", n);
  std::lock_guard<std::mutex> lk(o->mu);
  for (int i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= o->max_streams)
      return fail(WEKWS_HIP_EINVAL, "resample_bank_reset: stream %d outside 0..%d", ids[i], o->max_streams - 1);
  for (int i = 0; i < n; ++i) {
    const int id = ids[i];
    o->received[id] = 0; o->emitted[id] = 0; o->origin[id] = 0; o->flushed[id] = 0;
  }
  return WEKWS_HIP_OK;
}

int wekws_hip_resample_bank_counts(void* h, int id, int64_t counts_out[4]) {
  Bank* o = static_cast<Bank*>(h);
  if (!o || !counts_out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (id < 0 || id >= o->max_streams) return fail(WEKWS_HIP_EINVAL, "resample_bank_counts: stream %d outside 0..%d", id, o->max_streams - 1);
  std::lock_guard<std::mutex> lk(o->mu);
  counts_out[0] = o->received[id]; counts_out[1] = o->emitted[id];
  counts_out[2] = o->received[id] - o->origin[id]; counts_out[3] = o->flushed[id];
  return WEKWS_HIP_OK;
}

}  // extern "C"
