// Launchers, handle and C ABI of the streaming front end (stream_frontend.hip.h, stream_frontend.h).
#include "stream_frontend.hip.h"

namespace wekws {

int launch_fbank_stream(const FbankParams& P, const StreamFeRow* rows, const int16_t* pcm, int B, int nmax, int Tv, int16_t* lo,
                        float* dst, int resident, const float* dct, int num_ceps, hipStream_t stream) {
  const int rounds = (P.nslots + 63) / 64;
  if (rounds < 1 || rounds > 3) return -4;
  const int64_t total = int64_t(B) * Tv;
  int64_t grid = (total + kFbankWaves - 1) / kFbankWaves;
  if (resident > 0 && grid > resident) grid = resident;        // persistent waves: one resident round, like fbank_kernel
  const int pair_static = (P.frame_shift % 2 == 0) && (P.frame_length % 2 == 0) && (nmax % 2 == 0) &&
                          (reinterpret_cast<uintptr_t>(pcm) % 4 == 0) && (reinterpret_cast<uintptr_t>(lo) % 4 == 0);
  hipLaunchKernelGGL(fbank_stream_instance(rounds, dct != nullptr), dim3(unsigned(grid)), dim3(64 * kFbankWaves), fbank_stream_lds(),
                     stream, P, rows, pcm, B, nmax, Tv, lo, dst, pair_static, dct, num_ceps);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_splice_stream(const StreamFeRow* rows, const float* fresh, float* frs, float* out, int B, int max_items_f, int F,
                         int left, int W, int skip, hipStream_t stream) {
  const bool v4 = (F % 4 == 0) && (reinterpret_cast<uintptr_t>(fresh) % 16 == 0) && (reinterpret_cast<uintptr_t>(frs) % 16 == 0) &&
                  (reinterpret_cast<uintptr_t>(out) % 16 == 0);
  const int Fv = v4 ? F / 4 : F;
  const int items = v4 ? max_items_f / 4 : max_items_f;       // (items of a row are whole frames: a multiple of F)
  const dim3 grid(unsigned(B), unsigned((items + 255) / 256));
  if (v4)
    hipLaunchKernelGGL(splice_stream_kernel<float4>, grid, dim3(256), 0, stream, rows, reinterpret_cast<const float4*>(fresh),
                       reinterpret_cast<float4*>(frs), reinterpret_cast<float4*>(out), Fv, left, W, skip);
  else
    hipLaunchKernelGGL(splice_stream_kernel<float>, grid, dim3(256), 0, stream, rows, fresh, frs, out, Fv, left, W, skip);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace wekws

// ------------------------------------------------------------------------------------------------ C ABI
#include <mutex>
#include <new>
#include <vector>

#include "host_util.h"

namespace {

struct StreamFe {
  int device = 0;
  wekws::StreamFeCfg cfg{};
  wekws::FbankParams fp{};
  int max_streams = 0, max_chunk = 0;
  int F = 0, W = 1, keep = 0;          // floats of a frame (bins, or cepstra in MFCC mode), window of the context, frames remembered per stream
  int num_ceps = 0;                    // 0: log-mel rows
  float* d_dct = nullptr;              // MFCC mode: the (num_bins x num_ceps) DCT matrix with the lifter folded in (mfcc.hip.h)
  int rem_cap = 0;                     // samples per leftover buffer (even)
  int Tws = 1;                         // frame slots per row of the fresh-frame workspace
  bool direct = false;                 // no context, no skip: fbank writes the caller's rows
  int resident = 0;
  float* d_tables = nullptr;
  int16_t* lo = nullptr;               // (max_streams, 2, rem_cap) leftover samples, ping-ponged per stream
  float* frs = nullptr;                // (max_streams, 2, keep, F) remembered frames, ping-ponged per stream
  float* ws = nullptr;                 // (max_streams, Tws, F) fresh frames of a push
  // the plan table of a push travels through a ring of pinned host tables, each with its device twin and an event recorded
  // behind the push that used it: pushes queue back to back without a synchronise, a table is rewritten only once the copy out
  // of it has run (the host waits only with kStreamFeRing pushes still in flight)
  wekws::StreamFeRow* h_rows[wekws::kStreamFeRing] = {};
  wekws::StreamFeRow* d_rows[wekws::kStreamFeRing] = {};
  hipEvent_t ev[wekws::kStreamFeRing] = {};
  bool ev_used[wekws::kStreamFeRing] = {};
  int next = 0;
  std::mutex mu;
  // per-stream counts live on the host: the frames of every row are known without a device read-back
  std::vector<int32_t> rem, fr, off, lo_par, fr_par, seen;
  std::vector<int64_t> frames_total;
  int32_t epoch = 0;
  std::vector<wekws::StreamFePlan> plans;   // of the push being planned
};

int check_cfg(const wekws_hip_stream_frontend_cfg* c, wekws::StreamFeCfg* out) {
  const wekws_hip_fbank_cfg& f = c->fbank;
  if (f.num_bins <= 0 || f.num_bins > wekws::kFbankMaxBins || f.sample_rate <= 0 || f.frame_length <= 0 || f.frame_shift <= 0 ||
      f.frame_length > wekws::kFbankMaxFft)
    return fail(WEKWS_HIP_EINVAL, "stream_frontend: fbank cfg out of range");
  if (f.window != WEKWS_HIP_WINDOW_HAMMING && f.window != WEKWS_HIP_WINDOW_POVEY)
    return fail(WEKWS_HIP_EINVAL, "stream_frontend: fbank window %d", f.window);
  out->frame_length = f.frame_length; out->frame_shift = f.frame_shift;
  out->left = c->left; out->right = c->right; out->skip = c->skip;
  if (c->left != c->right)
    return fail(WEKWS_HIP_EINVAL, "stream_frontend: left %d != right %d -- the streaming reference is coherent only for left == right "
                "(left > right raises in its window loop, left < right drops frames)", c->left, c->right);
  if (wekws::stream_fe_cfg_ok(*out))
    return fail(WEKWS_HIP_EINVAL, "stream_frontend: frame_shift %d (1 .. frame_length %d) left %d right %d skip %d", f.frame_shift,
                f.frame_length, c->left, c->right, c->skip);
  return WEKWS_HIP_OK;
}

}  // namespace

extern "C" {

int wekws_hip_stream_frontend_plan(const wekws_hip_stream_frontend_cfg* cfg, const int32_t counts_in[3], int nsamp,
                                   int32_t plan_out[10]) {
  if (!cfg || !counts_in || !plan_out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  wekws::StreamFeCfg c{};
  if (int rc = check_cfg(cfg, &c)) return rc;
  const wekws::StreamFeCounts in{counts_in[0], counts_in[1], counts_in[2]};
  if (nsamp < 0 || in.rem < 0 || in.rem >= wekws::stream_fe_rem_cap(c) || in.fr < -1 || in.fr > c.left + c.right || in.off < 0 ||
      in.off >= c.skip)
    return fail(WEKWS_HIP_EINVAL, "stream_frontend_plan: nsamp=%d rem=%d fr=%d off=%d", nsamp, in.rem, in.fr, in.off);
  const wekws::StreamFePlan p = wekws::stream_fe_plan(c, in, nsamp);
  const int32_t v[wekws::kStreamFePlanInts] = {p.status, p.held, p.nf, p.rem_out, p.pad_first, p.fr_in, p.rows_ctx, p.rows_out,
                                               p.fr_out, p.off_out};
  for (int i = 0; i < wekws::kStreamFePlanInts; ++i) plan_out[i] = v[i];
  return WEKWS_HIP_OK;
}

void wekws_hip_stream_frontend_destroy(void* h) {
  StreamFe* o = static_cast<StreamFe*>(h);
  if (!o) return;
  DeviceGuard g(o->device);
  (void)hipDeviceSynchronize();
  for (int i = 0; i < wekws::kStreamFeRing; ++i) {
    if (o->ev[i]) (void)hipEventDestroy(o->ev[i]);
    if (o->h_rows[i]) (void)hipHostFree(o->h_rows[i]);
    if (o->d_rows[i]) (void)hipFree(o->d_rows[i]);
  }
  if (o->d_tables) (void)hipFree(o->d_tables);
  if (o->d_dct) (void)hipFree(o->d_dct);
  if (o->lo) (void)hipFree(o->lo);
  if (o->frs) (void)hipFree(o->frs);
  if (o->ws) (void)hipFree(o->ws);
  delete o;
}

// num_ceps 0: log-mel rows (wekws_hip_stream_frontend_create)
static int stream_frontend_create(const wekws_hip_stream_frontend_cfg* cfg, int num_ceps, float lifter, void** out) {
  wekws::StreamFeCfg c{};
  if (int rc = check_cfg(cfg, &c)) return rc;
  if (cfg->fbank.frame_length <= 64)
    return fail(WEKWS_HIP_EUNSUPPORTED, "fbank frame_length %d: frames of 65 .. 512 samples are built", cfg->fbank.frame_length);
  if (cfg->max_streams < 1 || cfg->max_chunk < 1)
    return fail(WEKWS_HIP_EINVAL, "stream_frontend: max_streams=%d max_chunk=%d", cfg->max_streams, cfg->max_chunk);
  const int64_t cap = (wekws::stream_fe_rem_cap(c) + 1) & ~int64_t(1);
  const int64_t Tws = wekws::stream_fe_max_nf(c, cfg->max_chunk) > 1 ? wekws::stream_fe_max_nf(c, cfg->max_chunk) : 1;
  const int keep = c.left + c.right;
  if (cap * 2 * cfg->max_streams > 0x7fffffffLL || Tws * cfg->max_streams > 0x7fffffffLL ||
      int64_t(keep > 0 ? keep : 1) * 2 * cfg->max_streams > 0x7fffffffLL || int64_t(cfg->max_chunk) + cap > 0x3fffffffLL)
    return fail(WEKWS_HIP_EINVAL, "stream_frontend: max_streams %d x max_chunk %d is out of range", cfg->max_streams, cfg->max_chunk);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev)
    return fail(WEKWS_HIP_EDEVICE, "device %d of %d", cfg->device, ndev);
  StreamFe* o = new (std::nothrow) StreamFe;
  if (!o) return fail(WEKWS_HIP_ENOMEM, "host allocation failed");
  o->device = cfg->device;
  o->cfg = c;
  o->max_streams = cfg->max_streams; o->max_chunk = cfg->max_chunk;
  o->num_ceps = num_ceps;
  o->F = num_ceps > 0 ? num_ceps : cfg->fbank.num_bins; o->W = keep + 1; o->keep = keep;
  o->rem_cap = int(cap); o->Tws = int(Tws);
  o->direct = keep == 0 && c.skip == 1;
  std::vector<float> tables;
  const int empty = wekws::fbank_build_tables(cfg->fbank.num_bins, cfg->fbank.sample_rate, cfg->fbank.frame_length,
                                              cfg->fbank.frame_shift, cfg->fbank.window, &o->fp, &tables);
  if (empty >= 0) {
    delete o;
    return fail(WEKWS_HIP_EINVAL, "fbank: mel filter %d of %d covers no FFT bin (sample_rate %d, frame_length %d): fewer bins", empty,
                cfg->fbank.num_bins, cfg->fbank.sample_rate, cfg->fbank.frame_length);
  }
  const size_t n = size_t(cfg->max_streams);
  o->rem.assign(n, 0); o->fr.assign(n, -1); o->off.assign(n, 0); o->lo_par.assign(n, 0); o->fr_par.assign(n, 0);
  o->seen.assign(n, 0); o->frames_total.assign(n, 0);
  o->plans.reserve(n);
  DeviceGuard g(cfg->device);
  hipError_t e = hipMalloc(&o->d_tables, tables.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(o->d_tables, tables.data(), tables.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess && num_ceps > 0) e = hipMalloc(&o->d_dct, size_t(cfg->fbank.num_bins) * num_ceps * sizeof(float));
  if (e == hipSuccess && num_ceps > 0 && wekws::build_dct_lifter_matrix(o->d_dct, cfg->fbank.num_bins, num_ceps, lifter, nullptr))
    e = hipGetLastError();
  if (e == hipSuccess) e = hipMalloc(&o->lo, n * 2 * size_t(cap) * sizeof(int16_t));
  if (e == hipSuccess) e = hipMemset(o->lo, 0, n * 2 * size_t(cap) * sizeof(int16_t));
  if (e == hipSuccess && keep > 0) e = hipMalloc(&o->frs, n * 2 * size_t(keep) * o->F * sizeof(float));
  if (e == hipSuccess && !o->direct) e = hipMalloc(&o->ws, n * size_t(Tws) * o->F * sizeof(float));
  for (int i = 0; i < wekws::kStreamFeRing && e == hipSuccess; ++i) {
    e = hipHostMalloc(&o->h_rows[i], n * sizeof(wekws::StreamFeRow), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&o->d_rows[i], n * sizeof(wekws::StreamFeRow));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&o->ev[i], hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = hip_fail(e, "stream_frontend create");
    wekws_hip_stream_frontend_destroy(o);
    return rc;
  }
  o->fp.tables = o->d_tables;
  o->resident = wekws::fbank_stream_resident_groups(o->fp, num_ceps > 0);
  *out = o;
  return WEKWS_HIP_OK;
}

int wekws_hip_stream_frontend_create(const wekws_hip_stream_frontend_cfg* cfg, void** out) {
  if (!cfg || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  return stream_frontend_create(cfg, 0, 0.f, out);
}

int wekws_hip_stream_frontend_create_mfcc(const wekws_hip_stream_frontend_cfg* cfg, int num_ceps, float cepstral_lifter, void** out) {
  if (!cfg || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  if (num_ceps <= 0 || num_ceps > cfg->fbank.num_bins || cfg->fbank.num_bins > wekws::kFbankMaxBins || !(cepstral_lifter >= 0.f))
    return fail(WEKWS_HIP_EINVAL, "stream_frontend: num_ceps=%d num_bins=%d lifter=%g (need 0 < num_ceps <= num_bins <= %d, lifter >= 0)",
                num_ceps, cfg->fbank.num_bins, double(cepstral_lifter), wekws::kFbankMaxBins);
  return stream_frontend_create(cfg, num_ceps, cepstral_lifter, out);
}

int wekws_hip_stream_frontend_max_frames(void* h, int nmax) {
  StreamFe* o = static_cast<StreamFe*>(h);
  if (!o || nmax < 0) return 0;
  return int(wekws::stream_fe_max_rows(o->cfg, nmax));
}

int wekws_hip_stream_frontend_push(void* h, const int16_t* pcm, int B, int nmax, const int32_t* stream_ids, const int32_t* nsamp,
                                   float* feats, int Tcap, int32_t* frames, void* stream_) {
  StreamFe* o = static_cast<StreamFe*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (B < 0 || nmax < 0 || Tcap < 0) return fail(WEKWS_HIP_EINVAL, "stream_frontend_push: B=%d nmax=%d Tcap=%d", B, nmax, Tcap);
  if (B == 0) return WEKWS_HIP_OK;
  if (!stream_ids || !nsamp || !frames || (nmax > 0 && !pcm)) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (nmax > o->max_chunk) return fail(WEKWS_HIP_EINVAL, "stream_frontend_push: nmax %d > max_chunk %d", nmax, o->max_chunk);
  if (B > o->max_streams) return fail(WEKWS_HIP_EINVAL, "stream_frontend_push: %d rows for %d streams", B, o->max_streams);
  if (int64_t(B) * Tcap > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "stream_frontend_push: B %d x Tcap %d is out of range", B, Tcap);
  std::lock_guard<std::mutex> lk(o->mu);
  // ---- the whole call is planned first: a refusal launches nothing and changes no state
  if (++o->epoch == 0x7fffffff) { o->epoch = 1; o->seen.assign(o->seen.size(), 0); }
  o->plans.clear();
  int Tv = 1, max_items = 0, need_cap = 0;
  for (int b = 0; b < B; ++b) {
    const int id = stream_ids[b];
    if (id < 0 || id >= o->max_streams) return fail(WEKWS_HIP_EINVAL, "stream_frontend_push: row %d: stream %d outside 0..%d", b, id, o->max_streams - 1);
    if (o->seen[id] == o->epoch) return fail(WEKWS_HIP_EINVAL, "stream_frontend_push: row %d: stream %d is given twice", b, id);
    o->seen[id] = o->epoch;
    if (nsamp[b] < 0 || nsamp[b] > nmax) return fail(WEKWS_HIP_EINVAL, "stream_frontend_push: row %d: %d samples outside 0..%d", b, nsamp[b], nmax);
    const wekws::StreamFePlan p = wekws::stream_fe_plan(o->cfg, wekws::StreamFeCounts{o->rem[id], o->fr[id], o->off[id]}, nsamp[b]);
    if (p.status)
      return fail(WEKWS_HIP_EINVAL, "stream_frontend_push: row %d (stream %d): %d frames for a right context of %d -- the reference "
                  "asserts more frames than its right context per chunk", b, id, p.nf, o->cfg.right);
    if (p.rem_out > o->rem_cap || p.nf > o->Tws) return fail(WEKWS_HIP_EINVAL, "stream_frontend_push: internal: plan outside the handle's buffers");
    if (p.rows_out > need_cap) need_cap = p.rows_out;
    if (p.nf > Tv) Tv = p.nf;
    const int items = (p.rows_out * o->W + (p.held || !o->keep ? 0 : p.fr_out)) * o->F;
    if (items > max_items) max_items = items;
    o->plans.push_back(p);
  }
  if (need_cap > Tcap) return fail(WEKWS_HIP_EINVAL, "stream_frontend_push: a row yields %d frames, Tcap is %d", need_cap, Tcap);
  if (need_cap > 0 && !feats) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  // ---- the plan table, in stream order
  DeviceGuard g(o->device);
  const hipStream_t s = static_cast<hipStream_t>(stream_);
  const int slot = o->next;
  o->next = (slot + 1) % wekws::kStreamFeRing;
  if (o->ev_used[slot]) {
    const hipError_t e = hipEventSynchronize(o->ev[slot]);
    if (e != hipSuccess) return hip_fail(e, "stream_frontend_push: plan ring");
  }
  wekws::StreamFeRow* rows = o->h_rows[slot];
  for (int b = 0; b < B; ++b) {
    const int id = stream_ids[b];
    const wekws::StreamFePlan& p = o->plans[b];
    const bool ctx = o->keep > 0 && !p.held;
    wekws::StreamFeRow& R = rows[b];
    R.rem = o->rem[id]; R.n = nsamp[b]; R.nf = p.nf; R.rem_out = p.rem_out;
    R.lo_old = (id * 2 + o->lo_par[id]) * o->rem_cap;
    R.lo_new = (id * 2 + (o->lo_par[id] ^ 1)) * o->rem_cap;
    R.fb_base = o->direct ? b * Tcap : b * o->Tws;
    R.pad_first = ctx ? p.pad_first : 1;                    // (no context: left = 0, the fresh frames themselves)
    R.fr_in = ctx ? p.fr_in : 0;
    R.fr_keep = ctx ? p.fr_out : 0;
    R.rows_out = p.rows_out; R.off = o->off[id];
    R.fr_old = (id * 2 + o->fr_par[id]) * o->keep;
    R.fr_new = (id * 2 + (o->fr_par[id] ^ 1)) * o->keep;
    R.out_base = b * Tcap;
    R.reserved = 0;
  }
  hipError_t e = hipMemcpyAsync(o->d_rows[slot], rows, size_t(B) * sizeof(wekws::StreamFeRow), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_fail(e, "stream_frontend_push: plan upload");
  // ---- two launches; from here the streams' state moves
  int rc = wekws::launch_fbank_stream(o->fp, o->d_rows[slot], pcm, B, nmax, Tv, o->lo, o->direct ? feats : o->ws, o->resident, o->d_dct,
                                      o->num_ceps, s);
  if (!rc && !o->direct && max_items > 0)
    rc = wekws::launch_splice_stream(o->d_rows[slot], o->ws, o->frs, feats, B, max_items, o->F, o->cfg.left, o->W, o->cfg.skip, s);
  e = hipEventRecord(o->ev[slot], s);
  o->ev_used[slot] = e == hipSuccess;
  for (int b = 0; b < B; ++b) {
    const int id = stream_ids[b];
    const wekws::StreamFePlan& p = o->plans[b];
    o->rem[id] = p.rem_out; o->fr[id] = p.fr_out; o->off[id] = p.off_out;
    o->lo_par[id] ^= 1;
    if (o->keep > 0 && !p.held) o->fr_par[id] ^= 1;
    if (p.rows_out > 0) o->frames_total[id] += p.rows_out;
    frames[b] = p.held ? -1 : p.rows_out;
  }
  if (rc) return hip_fail(hipGetLastError(), "stream_frontend_push launch");
  if (e != hipSuccess) return hip_fail(e, "stream_frontend_push: event");
  return WEKWS_HIP_OK;
}

int wekws_hip_stream_frontend_reset(void* h, const int32_t* ids, int n) {
  StreamFe* o = static_cast<StreamFe*>(h);
  if (!o) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (n < 0 || (n > 0 && !ids)) return fail(WEKWS_HIP_EINVAL, "stream_frontend_reset: n=%d", n);
  std::lock_guard<std::mutex> lk(o->mu);
  for (int i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= o->max_streams)
      return fail(WEKWS_HIP_EINVAL, "stream_frontend_reset: stream %d outside 0..%d", ids[i], o->max_streams - 1);
  // the counts ARE the state: a stream without samples, frames or phase reads nothing of its device buffers
  for (int i = 0; i < n; ++i) {
    const int id = ids[i];
    o->rem[id] = 0; o->fr[id] = -1; o->off[id] = 0; o->frames_total[id] = 0;
  }
  return WEKWS_HIP_OK;
}

int wekws_hip_stream_frontend_counts(void* h, int id, int32_t counts_out[4]) {
  StreamFe* o = static_cast<StreamFe*>(h);
  if (!o || !counts_out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (id < 0 || id >= o->max_streams) return fail(WEKWS_HIP_EINVAL, "stream_frontend_counts: stream %d outside 0..%d", id, o->max_streams - 1);
  std::lock_guard<std::mutex> lk(o->mu);
  counts_out[0] = o->rem[id]; counts_out[1] = o->fr[id]; counts_out[2] = o->off[id];
  counts_out[3] = int32_t(o->frames_total[id] > 0x7fffffffLL ? 0x7fffffffLL : o->frames_total[id]);
  return WEKWS_HIP_OK;
}

}  // extern "C"
