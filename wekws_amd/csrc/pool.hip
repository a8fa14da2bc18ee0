// The pool of stream caches and wekws_hip_forward_streams: the model stepped for many streams in one call.  Host side only.
#include <algorithm>
#include <new>

#include "model.h"
#include "ds256_stream.hip.h"

// ------------------------------------------------------------------------------------------------ the pool of stream caches
// (2, max_streams, E) floats, E = wekws_hip_cache_elems(m, 1): every stream has two planes, one of them live.  A step reads
// a stream's live plane and writes its other one, then the host flips the stream's parity bit -- in call order, which is stream
// order.  No kernel ever reads and writes the same bytes, so wekws_hip_forward's out_cache contract (no aliasing) holds as it is.
// A plane holds one stream's cache in wekws_hip_forward's geometry for B = 1; all zeros is the empty-cache sentinel.
constexpr int kPoolRing = 4;
struct wekws_hip_stream_cache {
  wekws_hip_model* m = nullptr;
  int device = 0, max_streams = 0;
  size_t E = 0;                          // floats of one plane
  float* planes = nullptr;
  std::vector<uint8_t> par;              // per stream: which plane is live
  std::vector<int32_t> seen;             // duplicate check of a call (epoch stamps)
  int32_t epoch = 0;
  // the row table of a call travels through a ring of pinned host tables, each with its device twin and an event recorded
  // behind the call that used it (like the streaming front end's): [max_streams StreamRow | max_streams FsmnGroup]
  char* h_tab[kPoolRing] = {};
  char* d_tab[kPoolRing] = {};
  hipEvent_t ev[kPoolRing] = {};
  bool ev_used[kPoolRing] = {};
  int next = 0;
  size_t groups_off = 0, tab_bytes = 0;
  // grouped path: the gathered features, caches and outputs of one bucket (grown on demand, one synchronisation)
  char* scratch = nullptr;
  size_t scratch_bytes = 0;
  std::vector<int32_t> order, gstart, gT;
  std::mutex mu;
  float* plane(int which, int id) const { return planes + (size_t(which) * max_streams + id) * E; }
};

static size_t pool_align(size_t v) { return (v + 255) / 256 * 256; }

// The buckets of a grouped call, one after the other on the stream: gather, the uniform forward, scatter
static int forward_streams_grouped(wekws_hip_model* m, wekws_hip_stream_cache* p, const wekws::StreamsPlan& plan,
                                   const wekws::StreamRow* d_rows, int softmax, hipStream_t stream) {
  const wekws_hip_desc& d = m->desc;
  const bool per_frame = per_frame_head(d);
  const int idim = d.idim, odim = d.odim;
  const int outer = d.backbone == WEKWS_HIP_BACKBONE_GRU ? d.num_layers : 1;      // (L, B, H) against (B, ...)
  const int inner = int(p->E / size_t(outer));
  auto bytes_of = [&](int nb, int n, size_t* xo, size_t* ci, size_t* co, size_t* yo) {
    size_t at = 0;
    *xo = at; at += pool_align(size_t(nb) * n * idim * sizeof(float));
    *ci = at; at += pool_align(size_t(nb) * p->E * sizeof(float));
    *co = at; at += pool_align(size_t(nb) * p->E * sizeof(float));
    *yo = at; at += pool_align(size_t(nb) * (per_frame ? size_t(n) * odim : size_t(odim)) * sizeof(float));
    return at;
  };
  size_t need = 0, xo, ci, co, yo;
  for (int g = 0; g < plan.ngroups; ++g) need = std::max(need, bytes_of(p->gstart[g + 1] - p->gstart[g], p->gT[g], &xo, &ci, &co, &yo));
  if (p->scratch_bytes < need) {
    if (p->scratch) {
      (void)hipStreamSynchronize(stream);                    // earlier calls may still use the old buffer
      (void)hipFree(p->scratch);
      p->scratch = nullptr; p->scratch_bytes = 0;
    }
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->scratch), need);
    if (e != hipSuccess) { p->scratch = nullptr; return fail(hip_code(e), "forward_streams: scratch of %zu bytes: %s", need, hipGetErrorString(e)); }
    p->scratch_bytes = need;
  }
  for (int g = 0; g < plan.ngroups; ++g) {
    const int nb = p->gstart[g + 1] - p->gstart[g], n = p->gT[g];
    (void)bytes_of(nb, n, &xo, &ci, &co, &yo);
    float* xg = reinterpret_cast<float*>(p->scratch + xo);
    float* cin = p->E ? reinterpret_cast<float*>(p->scratch + ci) : nullptr;
    float* cout = p->E ? reinterpret_cast<float*>(p->scratch + co) : nullptr;
    float* yg = reinterpret_cast<float*>(p->scratch + yo);
    const int xrow = n * idim, yrow = per_frame ? n * odim : odim;
    const int span = std::max(std::max(xrow, yrow), int(p->E));
    const dim3 grid(unsigned(nb), unsigned(std::min(16, (span + 1023) / 1024)));
    const wekws::StreamRow* rows = d_rows + p->gstart[g];
    if (!launch_pool_gather(grid, rows, nb, xg, xrow, cin, p->E ? outer : 0, inner, stream)) return fail(WEKWS_HIP_EDEVICE, "forward_streams: gather launch failed");
    if (const int rc = forward_call(m, xg, nb, n, cin, yg, cout, softmax, stream); rc != WEKWS_HIP_OK) return rc;
    if (!launch_pool_scatter(grid, rows, nb, yg, yrow, cout, p->E ? outer : 0, inner, stream)) return fail(WEKWS_HIP_EDEVICE, "forward_streams: scatter launch failed");
  }
  return WEKWS_HIP_OK;
}

extern "C" {

void wekws_hip_stream_cache_destroy(wekws_hip_stream_cache* p) {
  if (!p) return;
  DeviceGuard guard(p->device);
  (void)hipDeviceSynchronize();
  for (int i = 0; i < kPoolRing; ++i) {
    if (p->ev[i]) (void)hipEventDestroy(p->ev[i]);
    if (p->h_tab[i]) (void)hipHostFree(p->h_tab[i]);
    if (p->d_tab[i]) (void)hipFree(p->d_tab[i]);
  }
  if (p->planes) (void)hipFree(p->planes);
  if (p->scratch) (void)hipFree(p->scratch);
  delete p;
}

int wekws_hip_stream_cache_create(wekws_hip_model* m, int max_streams, wekws_hip_stream_cache** out) {
  if (!m || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  if (max_streams < 1) return fail(WEKWS_HIP_EINVAL, "stream_cache_create: max_streams=%d", max_streams);
  const size_t E = wekws_hip_cache_elems(m, 1);
  if (E > 0x7fffffffu || E * 2 * size_t(max_streams) > (size_t(1) << 40))
    return fail(WEKWS_HIP_EINVAL, "stream_cache_create: %d streams x %zu floats is out of range", max_streams, E);
  DeviceGuard guard(m->device);
  if (!guard.ok) return fail(WEKWS_HIP_EDEVICE, "hipSetDevice(%d)", m->device);
  wekws_hip_stream_cache* p = new (std::nothrow) wekws_hip_stream_cache();
  if (!p) return fail(WEKWS_HIP_ENOMEM, "host allocation");
  p->m = m; p->device = m->device; p->max_streams = max_streams; p->E = E;
  const size_t n = size_t(max_streams);
  p->par.assign(n, 0); p->seen.assign(n, 0);
  p->order.resize(n); p->gstart.resize(n + 1); p->gT.resize(n);
  p->groups_off = (n * sizeof(wekws::StreamRow) + 15) / 16 * 16;
  p->tab_bytes = p->groups_off + n * sizeof(wekws::FsmnGroup);
  const size_t plane_bytes = std::max<size_t>(2 * n * E, 1) * sizeof(float);
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->planes), plane_bytes);
  if (e == hipSuccess) e = hipMemset(p->planes, 0, plane_bytes);
  for (int i = 0; i < kPoolRing && e == hipSuccess; ++i) {
    e = hipHostMalloc(reinterpret_cast<void**>(&p->h_tab[i]), p->tab_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->d_tab[i]), p->tab_bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->ev[i], hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = fail(hip_code(e), "stream_cache_create: %s", hipGetErrorString(e));
    wekws_hip_stream_cache_destroy(p);
    return rc;
  }
  *out = p;
  return WEKWS_HIP_OK;
}

int wekws_hip_stream_cache_reset(wekws_hip_stream_cache* p, const int32_t* ids, int n, void* stream_) {
  if (!p) return fail(WEKWS_HIP_EINVAL, "NULL pool");
  if (ids && n < 0) return fail(WEKWS_HIP_EINVAL, "stream_cache_reset: n=%d", n);
  std::lock_guard<std::mutex> lk(p->mu);
  for (int i = 0; ids && i < n; ++i)
    if (ids[i] < 0 || ids[i] >= p->max_streams)
      return fail(WEKWS_HIP_EINVAL, "stream_cache_reset: stream %d outside 0..%d", ids[i], p->max_streams - 1);
  if (!p->E) return WEKWS_HIP_OK;
  DeviceGuard guard(p->device);
  if (!guard.ok) return fail(WEKWS_HIP_EDEVICE, "hipSetDevice(%d)", p->device);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  // zeros in the LIVE plane: the empty-cache sentinel of every backbone; the parity stays
  if (!ids) HIP_TRY(hipMemsetAsync(p->planes, 0, 2 * size_t(p->max_streams) * p->E * sizeof(float), stream));
  for (int i = 0; ids && i < n; ++i) HIP_TRY(hipMemsetAsync(p->plane(p->par[ids[i]], ids[i]), 0, p->E * sizeof(float), stream));
  return WEKWS_HIP_OK;
}

static int pool_copy(wekws_hip_stream_cache* p, int id, float* out, const float* in, void* stream_) {
  if (!p || (!out && !in)) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (id < 0 || id >= p->max_streams) return fail(WEKWS_HIP_EINVAL, "stream_cache: stream %d outside 0..%d", id, p->max_streams - 1);
  std::lock_guard<std::mutex> lk(p->mu);
  if (!p->E) return WEKWS_HIP_OK;
  DeviceGuard guard(p->device);
  if (!guard.ok) return fail(WEKWS_HIP_EDEVICE, "hipSetDevice(%d)", p->device);
  float* live = p->plane(p->par[id], id);
  HIP_TRY(hipMemcpyAsync(out ? out : live, out ? live : in, p->E * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream_)));
  return WEKWS_HIP_OK;
}
int wekws_hip_stream_cache_read(wekws_hip_stream_cache* p, int id, float* out, void* stream_) { return pool_copy(p, id, out, nullptr, stream_); }
int wekws_hip_stream_cache_write(wekws_hip_stream_cache* p, int id, const float* in, void* stream_) { return pool_copy(p, id, nullptr, in, stream_); }

int wekws_hip_forward_streams(wekws_hip_model* m, wekws_hip_stream_cache* p, const float* x, int B, int Tcap, const int32_t* stream_ids,
                              const int32_t* frames, float* y, int softmax, void* stream_) {
  if (!m || !p) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (p->m != m) return fail(WEKWS_HIP_EINVAL, "forward_streams: the pool was created for another model");
  if (B < 0 || Tcap <= 0) return fail(WEKWS_HIP_EINVAL, "forward_streams: B=%d Tcap=%d", B, Tcap);
  if (B == 0) return WEKWS_HIP_OK;
  if (!x || !y || !stream_ids || !frames) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (B > p->max_streams) return fail(WEKWS_HIP_EINVAL, "forward_streams: %d rows for %d streams", B, p->max_streams);
  const wekws_hip_desc& d = m->desc;
  const bool per_frame = per_frame_head(d);
  if (int64_t(B) * Tcap * std::max(d.idim, d.odim) > (int64_t(1) << 40)) return fail(WEKWS_HIP_EINVAL, "forward_streams: B %d x Tcap %d is out of range", B, Tcap);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::lock_guard<std::mutex> lk(p->mu);
  // ---- the whole call is checked first: a refusal launches nothing and changes no stream
  if (++p->epoch == 0x7fffffff) { p->epoch = 1; p->seen.assign(p->seen.size(), 0); }
  for (int b = 0; b < B; ++b) {
    const int id = stream_ids[b];
    if (id < 0 || id >= p->max_streams) return fail(WEKWS_HIP_EINVAL, "forward_streams: row %d: stream %d outside 0..%d", b, id, p->max_streams - 1);
    if (p->seen[id] == p->epoch) return fail(WEKWS_HIP_EINVAL, "forward_streams: row %d: stream %d is given twice", b, id);
    p->seen[id] = p->epoch;
    if (frames[b] > Tcap) return fail(WEKWS_HIP_EINVAL, "forward_streams: row %d: %d frames, Tcap is %d", b, frames[b], Tcap);
  }
  DeviceGuard guard(m->device);
  if (!guard.ok) return fail(WEKWS_HIP_EDEVICE, "hipSetDevice(%d)", m->device);
  if (stream_is_capturing(stream))
    return fail(WEKWS_HIP_EINVAL, "forward_streams: the row table travels from host memory that the next call rewrites: not inside a stream capture");
  trace_reset(m->generic ? kTraceAnyShape : kTraceOther);
  // ---- the plan (route.h): one table-driven launch, or buckets
  const wekws::StreamsPlan plan = wekws::plan_streams(d, m->rf, m->ro, m->fplan, !m->generic && !m->user_hdim && p->E % 4 == 0, m->cus, B, Tcap,
                                                      frames, p->order.data(), p->gstart.data(), p->gT.data());
  if (!plan.live) return WEKWS_HIP_OK;
  // ---- the row table, in stream order through the ring
  const int slot = p->next;
  p->next = (slot + 1) % kPoolRing;
  if (p->ev_used[slot]) HIP_TRY(hipEventSynchronize(p->ev[slot]));
  wekws::StreamRow* rows = reinterpret_cast<wekws::StreamRow*>(p->h_tab[slot]);
  wekws::FsmnGroup* groups = reinterpret_cast<wekws::FsmnGroup*>(p->h_tab[slot] + p->groups_off);
  for (int i = 0; i < plan.live; ++i) {
    const int b = p->order[i], id = stream_ids[b];
    wekws::StreamRow& R = rows[i];
    R.x = x + size_t(b) * Tcap * d.idim;
    R.in_cache = p->plane(p->par[id], id);
    R.out_cache = p->plane(p->par[id] ^ 1, id);
    R.y = per_frame ? y + size_t(b) * Tcap * d.odim : y + size_t(b) * d.odim;
    R.T = frames[b];
    R.yrows = per_frame ? frames[b] : 1;
  }
  size_t up = size_t(plan.live) * sizeof(wekws::StreamRow);
  if (plan.kind == wekws::STREAMS_FSMN) {
    for (int g = 0; g < plan.ngroups; ++g) {
      wekws::FsmnGroup& G = groups[g];
      G = wekws::FsmnGroup{};
      G.T = p->gT[g];
      for (int k = 0; k < 4; ++k) G.row[k] = p->gstart[g] + k < p->gstart[g + 1] ? p->gstart[g] + k : -1;
    }
    up = p->groups_off + size_t(plan.ngroups) * sizeof(wekws::FsmnGroup);
  }
  HIP_TRY(hipMemcpyAsync(p->d_tab[slot], p->h_tab[slot], up, hipMemcpyHostToDevice, stream));
  const wekws::StreamRow* d_rows = reinterpret_cast<const wekws::StreamRow*>(p->d_tab[slot]);
  const wekws::FsmnGroup* d_groups = reinterpret_cast<const wekws::FsmnGroup*>(p->d_tab[slot] + p->groups_off);
  // ---- the launches; from here the streams' state moves
  int rc = WEKWS_HIP_OK;
  const bool sm = softmax || d.activation == WEKWS_HIP_ACT_SOFTMAX;
  if (plan.kind == wekws::STREAMS_DS256) {
    wekws::CallArgs a{};
    a.x = x; a.xs_b = int64_t(Tcap) * d.idim;
    a.in_cache = p->planes; a.out_cache = p->planes;         // (never read: every row brings its own planes)
    a.y = y; a.ys_b = per_frame ? int64_t(Tcap) * d.odim : d.odim;
    a.B = plan.live; a.T = plan.max_T; a.T_total = plan.max_T;
    a.first_tile = a.last_tile = 1;
    a.head_slices = plan.conv.head_slices;
    a.nf = m->nf_dev;
    a.rows = d_rows;
    trace(kTraceConv, plan.conv);
    const int lr = wekws::launch_ds256_stream_rows(plan.conv, m->sp, a, stream);
    if (lr == -4) rc = fail(WEKWS_HIP_EUNSUPPORTED, "internal: ds256_stream has no table-driven kernel for the route");
    else if (lr) rc = fail(lr, "forward_streams: ds256_stream launch failed: %s", hipGetErrorString(hipGetLastError()));
  } else if (plan.kind == wekws::STREAMS_FSMN) {
    wekws::FsmnArgs a{};
    a.x = x; a.xs_b = int64_t(Tcap) * d.idim;
    a.in_cache = p->planes; a.out_cache = p->planes;         // (never read: every row brings its own planes)
    a.y = y; a.ys_b = int64_t(Tcap) * d.odim;
    a.B = plan.live; a.T = plan.max_T;
    a.head_slices = plan.fsmn.head_slices;
    a.nf = m->nf_dev;
    a.rows = d_rows; a.groups = d_groups;
    trace(kTraceFsmn, plan.fsmn);
    const int lr = wekws::launch_fsmn_f16_rows(plan.fsmn, m->fq, a, stream);
    if (lr == -4) rc = fail(WEKWS_HIP_EUNSUPPORTED, "internal: the FSMN kernel has no table-driven instance for the route (nt=%d u=%d)", plan.fsmn.nt, plan.fsmn.u);
    else if (lr) rc = fail(lr, "forward_streams: fsmn launch failed: %s", hipGetErrorString(hipGetLastError()));
  } else {
    rc = forward_streams_grouped(m, p, plan, d_rows, softmax, stream);
  }
  if (!rc && sm && plan.kind != wekws::STREAMS_GROUPED &&
      !wekws::launch_softmax_stream_rows(d_rows, plan.live, per_frame ? plan.max_T : 1, d.odim, stream))
    rc = fail(WEKWS_HIP_EDEVICE, "forward_streams: softmax launch failed");
  const hipError_t ee = hipEventRecord(p->ev[slot], stream);
  p->ev_used[slot] = ee == hipSuccess;
  if (rc) return rc;
  for (int i = 0; i < plan.live; ++i) p->par[stream_ids[p->order[i]]] ^= 1;
  if (ee != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "forward_streams: event: %s", hipGetErrorString(ee));
  return WEKWS_HIP_OK;
}

}  // extern "C"
