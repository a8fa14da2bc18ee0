// Launchers, handles and C ABI of the augmentation stages (augment.hip.h, augment_plan.h).
#include "augment.hip.h"

#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "host_util.h"

namespace {

constexpr int kRing = 4;

// Per-row tables reach the device in stream order without a synchronisation: a ring of pinned host tables with device twins,
// each with an event recorded behind the call that used it (as the resampler's).  The host waits only for the call that used
// the slot kRing calls ago; a slot too small for a call is replaced behind that wait, so no launch still reads it.
struct TableRing {
  struct Slot {
    void* h = nullptr;
    void* d = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool used = false;
  };
  Slot slots[kRing];
  int next = 0;

  int acquire(size_t bytes, hipStream_t s, Slot** out) {
    Slot& slot = slots[next];
    if (slot.used) {
      HIP_TRY(hipEventSynchronize(slot.ev));
      slot.used = false;
    }
    if (bytes > slot.cap) {
      if (stream_is_capturing(s)) return fail(WEKWS_HIP_EINVAL, "augment: %zu bytes of row tables need a larger slot: not inside a capture", bytes);
      if (slot.h) (void)hipHostFree(slot.h);
      if (slot.d) (void)hipFree(slot.d);
      slot.h = nullptr; slot.d = nullptr; slot.cap = 0;
      HIP_TRY(hipHostMalloc(&slot.h, bytes, hipHostMallocDefault));
      HIP_TRY(hipMalloc(&slot.d, bytes));
      if (!slot.ev) HIP_TRY(hipEventCreateWithFlags(&slot.ev, hipEventDisableTiming));
      slot.cap = bytes;
    }
    next = (next + 1) % kRing;
    *out = &slot;
    return WEKWS_HIP_OK;
  }
  static int upload(Slot* slot, size_t bytes, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(slot->d, slot->h, bytes, hipMemcpyHostToDevice, s));
    return WEKWS_HIP_OK;
  }
  static int done(Slot* slot, hipStream_t s) {
    const hipError_t e = hipEventRecord(slot->ev, s);
    slot->used = e == hipSuccess;
    return e == hipSuccess ? WEKWS_HIP_OK : hip_fail(e, "augment: event");
  }
  void destroy() {
    for (Slot& t : slots) {
      if (t.ev) (void)hipEventDestroy(t.ev);
      if (t.h) (void)hipHostFree(t.h);
      if (t.d) (void)hipFree(t.d);
      t = Slot{};
    }
  }
};

int max_grid_of(int device) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess || prop.multiProcessorCount <= 0) return 1024;
  return prop.multiProcessorCount * 3;             // 42.5 KB of LDS a workgroup: three fit a CU
}

int refusal(const char* what, int why, int row) {
  static const char* const text[] = {"", "a count or a size is out of range, or a table is NULL", "samples outside 0..nmax",
                                     "index outside -1..count-1", "start < 0, or start + samples past the end of a noise longer than the row",
                                     "snr_db is not finite", "pcm_scale is not a positive finite number",
                                     "a mask is not 0 <= start <= end <= the row's frames (time) or F (frequency)"};
  return fail(WEKWS_HIP_EINVAL, "%s: row %d: %s", what, row, text[why]);
}

int device_ok(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(WEKWS_HIP_EDEVICE, "device %d of %d", device, ndev);
  return WEKWS_HIP_OK;
}

// a bank of R rows of up to max_len samples with a length each: the shape's own check
int bank_check(const char* what, const float* bank, const int32_t* lengths, int R, int max_len) {
  if (!bank || !lengths) return fail(WEKWS_HIP_EINVAL, "%s: NULL argument", what);
  if (R < 1 || max_len < 1 || max_len > wekws::kAugmentMaxLen) return fail(WEKWS_HIP_EINVAL, "%s: %d rows of up to %d samples", what, R, max_len);
  for (int r = 0; r < R; ++r)
    if (lengths[r] <= 0 || lengths[r] > max_len) return fail(WEKWS_HIP_EINVAL, "%s: row %d: length %d outside 1..%d", what, r, lengths[r], max_len);
  return WEKWS_HIP_OK;
}

}  // namespace

struct wekws_hip_reverb {
  int device = 0, max_grid = 1;
  std::vector<int32_t> len, part_off, parts;      // of every RIR
  wekws::AugC* d_Hf = nullptr;                    // (sum of partitions, H + 1)
  wekws::AugC* d_tw = nullptr;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  TableRing ring;
  std::mutex mu;
};

struct wekws_hip_noise {
  int device = 0;
  std::vector<int32_t> len;
  std::vector<int64_t> off;
  float* d_bank = nullptr;
  TableRing ring;
  std::mutex mu;
};

extern "C" {

int wekws_hip_reverb_hop(void) { return wekws::kReverbHop; }

int wekws_hip_reverb_plan(int rir_len, int B, int nmax, int64_t out[4]) {
  if (!out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (rir_len < 1 || rir_len > wekws::kAugmentMaxLen || B < 0 || nmax < 0 || nmax > wekws::kAugmentMaxLen)
    return fail(WEKWS_HIP_EINVAL, "reverb_plan: rir_len=%d B=%d nmax=%d", rir_len, B, nmax);
  out[0] = wekws::reverb_partitions(rir_len);
  out[1] = wekws::reverb_blocks(nmax);
  out[2] = wekws::reverb_workspace_bytes(B, nmax);
  out[3] = wekws::reverb_spectra_bytes(rir_len);
  return WEKWS_HIP_OK;
}

int wekws_hip_reverb_check(const int32_t* rir_lengths, int R, int B, int nmax, const int32_t* nsamp, const int32_t* rir_of_row) {
  int row = -1;
  const int why = wekws::reverb_check(rir_lengths, R, B, nmax, nsamp, rir_of_row, &row);
  return why ? refusal("reverb_apply", why, row) : WEKWS_HIP_OK;
}

void wekws_hip_reverb_destroy(void* h) {
  wekws_hip_reverb* o = static_cast<wekws_hip_reverb*>(h);
  if (!o) return;
  DeviceGuard g(o->device);
  (void)hipDeviceSynchronize();
  o->ring.destroy();
  if (o->d_Hf) (void)hipFree(o->d_Hf);
  if (o->d_tw) (void)hipFree(o->d_tw);
  if (o->ws) (void)hipFree(o->ws);
  delete o;
}

int wekws_hip_reverb_create(const float* rirs, const int32_t* lengths, int R, int max_len, int device, void** out) {
  if (!out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  if (int rc = bank_check("reverb_create", rirs, lengths, R, max_len)) return rc;
  std::vector<double> scale(static_cast<size_t>(R));
  int64_t parts = 0;
  for (int r = 0; r < R; ++r) {
    const int bad = wekws::reverb_rir_scale(rirs + int64_t(r) * max_len, lengths[r], &scale[size_t(r)]);
    if (bad) return fail(WEKWS_HIP_EINVAL, "reverb_create: RIR %d %s", r, bad == 1 ? "holds a NaN or an Inf" : "is all zeros: it has no norm");
    parts += wekws::reverb_partitions(lengths[r]);
  }
  if (parts > 0x7fffffffLL / wekws::kReverbBins) return fail(WEKWS_HIP_EINVAL, "reverb_create: %lld partitions are out of range", (long long)parts);
  if (int rc = device_ok(device)) return rc;
  wekws_hip_reverb* o = new (std::nothrow) wekws_hip_reverb;
  if (!o) return fail(WEKWS_HIP_ENOMEM, "host allocation failed");
  o->device = device;
  std::vector<float> spectra;
  spectra.reserve(size_t(parts) * wekws::kReverbBins * 2);
  const std::vector<std::complex<double>> w = wekws::reverb_twiddles_host();
  int32_t at = 0;
  for (int r = 0; r < R; ++r) {
    o->len.push_back(lengths[r]);
    o->part_off.push_back(at);
    o->parts.push_back(int32_t(wekws::reverb_partitions(lengths[r])));
    at += o->parts.back();
    wekws::reverb_rir_spectra(rirs + int64_t(r) * max_len, lengths[r], scale[size_t(r)], w, &spectra);
  }
  std::vector<float> tw(size_t(wekws::kReverbTwiddles) * 2);
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < wekws::kReverbTwiddles; ++k) {
    tw[size_t(2) * k] = float(std::cos(-2.0 * pi * k / wekws::kReverbFft));
    tw[size_t(2) * k + 1] = float(std::sin(-2.0 * pi * k / wekws::kReverbFft));
  }
  DeviceGuard g(device);
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&o->d_Hf), spectra.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(o->d_Hf, spectra.data(), spectra.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&o->d_tw), tw.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(o->d_tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = hip_fail(e, "reverb create");
    wekws_hip_reverb_destroy(o);
    return rc;
  }
  o->max_grid = max_grid_of(device);
  *out = o;
  return WEKWS_HIP_OK;
}

size_t wekws_hip_reverb_workspace_bytes(void* h, int B, int nmax) {
  if (!h || B < 0 || nmax < 0 || nmax > wekws::kAugmentMaxLen) return 0;
  return size_t(wekws::reverb_workspace_bytes(B, nmax));
}

int wekws_hip_reverb_apply(void* h, const float* pcm, int B, int nmax, const int32_t* nsamp, const int32_t* rir_of_row, float* out,
                           void* stream_) {
  wekws_hip_reverb* o = static_cast<wekws_hip_reverb*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  int row = -1;
  if (const int why = wekws::reverb_check(o->len.data(), int(o->len.size()), B, nmax, nsamp, rir_of_row, &row))
    return refusal("reverb_apply", why, row);
  if (B == 0 || nmax == 0) return WEKWS_HIP_OK;
  if (!pcm || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (pcm == out) return fail(WEKWS_HIP_EINVAL, "reverb_apply: out must not be pcm (a block reads the samples of the block before it)");
  std::lock_guard<std::mutex> lk(o->mu);
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream_);
  const size_t need = size_t(wekws::reverb_workspace_bytes(B, nmax));
  if (need > o->ws_bytes) {
    if (stream_is_capturing(s)) return fail(WEKWS_HIP_EINVAL, "reverb_apply: %zu bytes of scratch need a larger workspace: not inside a capture", need);
    if (o->ws) (void)hipFree(o->ws);               // (synchronises: no launch still uses it)
    o->ws = nullptr; o->ws_bytes = 0;
    HIP_TRY(hipMalloc(&o->ws, need));
    o->ws_bytes = need;
  }
  TableRing::Slot* slot = nullptr;
  if (int rc = o->ring.acquire(size_t(B) * sizeof(wekws::ReverbRow), s, &slot)) return rc;
  wekws::ReverbRow* rows = static_cast<wekws::ReverbRow*>(slot->h);
  bool any = false;
  for (int b = 0; b < B; ++b) {
    const int n = nsamp ? nsamp[b] : nmax, r = rir_of_row[b];
    rows[b].n = n;
    rows[b].nblk = int32_t(wekws::reverb_blocks(n));
    rows[b].part_off = r < 0 ? 0 : o->part_off[size_t(r)];
    rows[b].P = r < 0 ? 0 : o->parts[size_t(r)];
    any |= r >= 0 && n > 0;
  }
  if (int rc = TableRing::upload(slot, size_t(B) * sizeof(wekws::ReverbRow), s)) return rc;
  const int nbmax = int(wekws::reverb_blocks(nmax));
  const int64_t total = int64_t(B) * nbmax;
  const unsigned grid = unsigned(total < o->max_grid ? total : o->max_grid);
  wekws::AugC* const X = static_cast<wekws::AugC*>(o->ws);
  int32_t* const bad = reinterpret_cast<int32_t*>(static_cast<char*>(o->ws) + wekws::reverb_flags_offset(B, nmax));
  const wekws::ReverbRow* const d_rows = static_cast<const wekws::ReverbRow*>(slot->d);
  hipError_t e = hipSuccess;
  if (any) {
    e = hipMemsetAsync(bad, 0, size_t(B) * sizeof(int32_t), s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(wekws::reverb_forward_kernel, dim3(grid), dim3(wekws::kAugThreads), wekws::kReverbLdsBytes, s, d_rows, pcm, nmax,
                         nbmax, o->d_tw, X, bad, total);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(wekws::reverb_inverse_kernel, dim3(grid), dim3(wekws::kAugThreads), wekws::kReverbLdsBytes, s, d_rows, pcm, nmax,
                       nbmax, o->d_tw, X, o->d_Hf, bad, out, total);
    e = hipGetLastError();
  }
  const int rc = TableRing::done(slot, s);
  if (e != hipSuccess) return hip_fail(e, "reverb_apply launch");
  return rc;
}

// ------------------------------------------------------------------------------------------------ noise
void wekws_hip_noise_destroy(void* h) {
  wekws_hip_noise* o = static_cast<wekws_hip_noise*>(h);
  if (!o) return;
  DeviceGuard g(o->device);
  (void)hipDeviceSynchronize();
  o->ring.destroy();
  if (o->d_bank) (void)hipFree(o->d_bank);
  delete o;
}

int wekws_hip_noise_create(const float* noises, const int32_t* lengths, int Rn, int max_len, int device, void** out) {
  if (!out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  if (int rc = bank_check("noise_create", noises, lengths, Rn, max_len)) return rc;
  if (int rc = device_ok(device)) return rc;
  wekws_hip_noise* o = new (std::nothrow) wekws_hip_noise;
  if (!o) return fail(WEKWS_HIP_ENOMEM, "host allocation failed");
  o->device = device;
  std::vector<float> bank;                          // the noises back to back: a length each, no padding
  for (int r = 0; r < Rn; ++r) {
    o->len.push_back(lengths[r]);
    o->off.push_back(int64_t(bank.size()));
    bank.insert(bank.end(), noises + int64_t(r) * max_len, noises + int64_t(r) * max_len + lengths[r]);
  }
  DeviceGuard g(device);
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&o->d_bank), bank.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(o->d_bank, bank.data(), bank.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = hip_fail(e, "noise create");
    wekws_hip_noise_destroy(o);
    return rc;
  }
  *out = o;
  return WEKWS_HIP_OK;
}

int wekws_hip_noise_check(const int32_t* noise_lengths, int Rn, int B, int nmax, const int32_t* nsamp, const int32_t* noise_of_row,
                          const int32_t* start, const double* snr_db, double pcm_scale) {
  int row = -1;
  const int why = wekws::noise_check(noise_lengths, Rn, B, nmax, nsamp, noise_of_row, start, snr_db, pcm_scale, &row);
  return why ? refusal("noise_mix", why, row) : WEKWS_HIP_OK;
}

int wekws_hip_noise_mix(void* h, const float* pcm, int B, int nmax, const int32_t* nsamp, const int32_t* noise_of_row, const int32_t* start,
                        const double* snr_db, double pcm_scale, float* out, void* stream_) {
  wekws_hip_noise* o = static_cast<wekws_hip_noise*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  int row = -1;
  if (const int why = wekws::noise_check(o->len.data(), int(o->len.size()), B, nmax, nsamp, noise_of_row, start, snr_db, pcm_scale, &row))
    return refusal("noise_mix", why, row);
  if (B == 0 || nmax == 0) return WEKWS_HIP_OK;
  if (!pcm || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  std::lock_guard<std::mutex> lk(o->mu);
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream_);
  TableRing::Slot* slot = nullptr;
  if (int rc = o->ring.acquire(size_t(B) * sizeof(wekws::NoiseRow), s, &slot)) return rc;
  wekws::NoiseRow* rows = static_cast<wekws::NoiseRow*>(slot->h);
  for (int b = 0; b < B; ++b) {
    const int r = noise_of_row[b];
    wekws::NoiseRow& R = rows[b];
    R = wekws::NoiseRow{};
    R.n = nsamp ? nsamp[b] : nmax;
    if (r < 0) continue;
    R.off = o->off[size_t(r)];
    R.nlen = o->len[size_t(r)];
    R.start = start[b] % R.nlen;
    R.snr_db = snr_db[b];
  }
  if (int rc = TableRing::upload(slot, size_t(B) * sizeof(wekws::NoiseRow), s)) return rc;
  hipLaunchKernelGGL(wekws::noise_mix_kernel, dim3(unsigned(B)), dim3(wekws::kAugThreads), 0, s, static_cast<const wekws::NoiseRow*>(slot->d),
                     pcm, nmax, o->d_bank, float(pcm_scale), out);
  const hipError_t e = hipGetLastError();
  const int rc = TableRing::done(slot, s);
  if (e != hipSuccess) return hip_fail(e, "noise_mix launch");
  return rc;
}

// ------------------------------------------------------------------------------------------------ masks
int wekws_hip_spec_mask(const float* feats, int B, int T, int F, const int32_t* lengths, const int32_t* t_masks, int nt,
                        const int32_t* f_masks, int nf, float* out, void* stream_) {
  int row = -1;
  if (const int why = wekws::spec_mask_check(B, T, F, lengths, t_masks, nt, f_masks, nf, &row)) return refusal("spec_mask", why, row);
  const int64_t total = int64_t(B) * T * F;
  if (total == 0) return WEKWS_HIP_OK;
  if (!feats || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, feats) != hipSuccess || attr.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return fail(WEKWS_HIP_EDEVICE, "spec_mask: feats is not device memory");
  }
  // the call has no handle: its tables travel through one ring per device, owned by the library
  static std::mutex mu;
  static TableRing rings[16];
  if (attr.device < 0 || attr.device >= 16) return fail(WEKWS_HIP_EDEVICE, "spec_mask: device %d", attr.device);
  std::lock_guard<std::mutex> lk(mu);
  DeviceGuard g(attr.device);
  const hipStream_t s = static_cast<hipStream_t>(stream_);
  const size_t words = size_t(B) * (1 + 2 * (size_t(nt) + size_t(nf)));
  TableRing::Slot* slot = nullptr;
  if (int rc = rings[attr.device].acquire(words * sizeof(int32_t), s, &slot)) return rc;
  int32_t* tab = static_cast<int32_t*>(slot->h);
  for (int b = 0; b < B; ++b) tab[b] = lengths ? lengths[b] : T;
  if (nt) std::memcpy(tab + B, t_masks, size_t(B) * nt * 2 * sizeof(int32_t));
  if (nf) std::memcpy(tab + B + size_t(B) * nt * 2, f_masks, size_t(B) * nf * 2 * sizeof(int32_t));
  if (int rc = TableRing::upload(slot, words * sizeof(int32_t), s)) return rc;
  const int64_t groups = (total + wekws::kAugThreads - 1) / wekws::kAugThreads;
  hipLaunchKernelGGL(wekws::spec_mask_kernel, dim3(unsigned(groups < 65536 ? groups : 65536)), dim3(wekws::kAugThreads), 0, s, feats, T, F,
                     static_cast<const int32_t*>(slot->d), B, nt, nf, out, total);
  const hipError_t e = hipGetLastError();
  const int rc = TableRing::done(slot, s);
  if (e != hipSuccess) return hip_fail(e, "spec_mask launch");
  return rc;
}

}  // extern "C"
