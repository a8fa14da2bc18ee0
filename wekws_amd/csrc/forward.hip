// wekws_hip_forward: the forward paths of the four backbones and the any-shape path -- the route of every launch (route.h), its
// scratch from the stream's workspace, the launcher of the route's family -- and reserve / status.  Host side only.
#include <cstdlib>

#include "model.h"
#include "ds256_w16.hip.h"
#include "ds256_g16.hip.h"
#include "ds256_g32.hip.h"
#include "mdtc64_g4.hip.h"
#include "ds64_g4.hip.h"
#include "ds256_stream.hip.h"
#include "ds256_mm.hip.h"
#include "mdtc64_w16.hip.h"
#include "mdtc64_stream.hip.h"
#include "gru_pipe.hip.h"

// (measurement aid: WEKWS_NF_FIX_ALL=1 runs the separate non-finite pass behind EVERY conv kernel, to price the extra launch)
static bool nf_fix_all() {
  static const bool v = [] { const char* e = std::getenv("WEKWS_NF_FIX_ALL"); return e && e[0] == '1'; }();
  return v;
}

// The GRU route of a call (route.h); x16: the features 16-byte aligned
static wekws::GruRoute gru_route(const wekws_hip_model* m, int B, int T, bool x16 = true) {
  return wekws::select_gru_route(m->desc, m->ro, wekws::GruCall{B, T, x16, m->user_hdim != 0, m->cus});
}
// Scratch bytes one wekws_hip_forward(m, B, T) takes from its stream's workspace (0: none): every path's come from its route /
// layout in route.h (generic.hip.h for the any-shape path), for the forward paths below and for wekws_hip_reserve alike ...
static size_t workspace_need(const wekws_hip_model* m, int B, int T) {
  const wekws_hip_desc& d = m->desc;
  if (B <= 0 || T <= 0) return 0;
  if (m->generic) return wekws::gen_workspace_bytes(m->gm, B, T);     // (monotonic in B and T)
  if (d.backbone == WEKWS_HIP_BACKBONE_FSMN) return wekws::select_fsmn_route(m->fplan, d, m->ro, B, T, 0, m->cus).ws_bytes;
  if (d.backbone == WEKWS_HIP_BACKBONE_GRU) return gru_route(m, B, T).plain_bytes;
  return wekws::conv_workspace(d, m->cache_len, B, T, m->user_hdim != 0).bytes;
}
// ... and the bytes of its granule buffer (the GRU wavefront: a second per-stream buffer that holds nothing else)
static size_t granule_need(const wekws_hip_model* m, int B, int T) {
  if (B <= 0 || T <= 0 || m->generic || m->desc.backbone != WEKWS_HIP_BACKBONE_GRU) return 0;
  return gru_route(m, B, T).granule_bytes;
}

// The frames of one FSMN call, cut into LDS tiles chained through ping-pong workspace caches
static int forward_fsmn(wekws_hip_model* m, const float* x, int B, int T, const float* in_cache, float* y,
                        float* out_cache, hipStream_t stream) {
  const wekws_hip_desc& d = m->desc;
  const wekws::FsmnRoute first = wekws::select_fsmn_route(m->fplan, d, m->ro, B, T, 0, m->cus);
  const int TILE = first.tile_frames, ntiles = first.ntiles;
  float* ws_cache[2] = {nullptr, nullptr};
  if (ntiles > 1) {
    char* base = stream_workspace(m, stream, first.ws_bytes);
    if (!base) return WEKWS_HIP_ENOMEM;
    ws_cache[0] = reinterpret_cast<float*>(base);
    ws_cache[1] = reinterpret_cast<float*>(base + first.ws_cache);
  }
  for (int i = 0; i < ntiles; ++i) {
    const int t0 = i * TILE;
    const int Tt = (T - t0 < TILE) ? (T - t0) : TILE;
    wekws::FsmnArgs a{};
    a.x = x + size_t(t0) * d.idim;
    a.xs_b = int64_t(T) * d.idim;
    a.in_cache = (i == 0) ? in_cache : ws_cache[(i - 1) & 1];
    a.out_cache = (i == ntiles - 1) ? out_cache : ws_cache[i & 1];
    a.y = y + size_t(t0) * d.odim;
    a.ys_b = int64_t(T) * d.odim;
    a.B = B;
    a.T = Tt;
    a.nf = m->nf_dev;
    // frame tiles, utterances per workgroup, head slices: route.h
    const wekws::FsmnRoute route = i == 0 ? first : wekws::select_fsmn_route(m->fplan, d, m->ro, B, T, i, m->cus);
    trace(kTraceFsmn, route);
    a.head_slices = route.head_slices;
    const int rc = wekws::launch_fsmn_f16(route, m->fq, a, stream);
    if (rc == -4) return fail(WEKWS_HIP_EUNSUPPORTED, "internal: the FSMN kernel has no instance for the route (nt=%d u=%d LDS %d)", route.nt, route.u, route.lds_bytes);
    if (rc) return fail(rc, "fsmn launch failed (nt=%d u=%d): %s", route.nt, route.u, hipGetErrorString(hipGetLastError()));
  }
  return WEKWS_HIP_OK;
}

// The any-shape path (generic.hip.h)
static int forward_generic(wekws_hip_model* m, const float* x, int B, int T, const float* in_cache, float* y, float* out_cache,
                           hipStream_t stream) {
  char* base = stream_workspace(m, stream, workspace_need(m, B, T));
  if (!base) return WEKWS_HIP_ENOMEM;
  hipError_t lerr = hipSuccess;
  const int rc = wekws::generic_forward(m->gm, x, B, T, in_cache, y, out_cache, base, stream, &lerr);
  if (rc) return fail(rc, "any-shape path: launch failed: %s", hipGetErrorString(lerr));
  return WEKWS_HIP_OK;
}

static int forward_gru(wekws_hip_model* m, const float* x, int B, int T, const float* in_cache, float* y, float* out_cache,
                       hipStream_t stream) {
  const wekws_hip_desc& d = m->desc;
  // a wavefront launch of an EARLIER call on this stream that gave up is reported here, by the call that follows it (one
  // read of host memory; the reference's forward either returns correct values or raises -- keyword_spotting.cc:77-79)
  int rc = stream_health(m, stream);
  if (rc) return rc;
  // ---- which kernels, their geometry and scratch: route.h (select_gru_route)
  const wekws::GruRoute route = gru_route(m, B, T, reinterpret_cast<uintptr_t>(x) % 16 == 0);
  if (route.family == wekws::GRU_NONE) return fail(WEKWS_HIP_EUNSUPPORTED, "no GRU kernel for this call: %s", route.why_not ? route.why_not : "?");
  trace(kTraceGru, route);
  // workspace: one grow-only buffer per (model, stream) -- calls on the same stream are ordered by the stream, calls on
  // different streams never share a buffer
  char* base = nullptr;
  if (route.plain_bytes && !(base = stream_workspace(m, stream, route.plain_bytes))) return WEKWS_HIP_ENOMEM;
  float* user_h_out = nullptr;
  if (m->user_hdim) {                                      // zero-padded hidden size: widened copies of the caller's states
    const size_t he = size_t(d.num_layers) * B * d.hdim;
    float* wide = reinterpret_cast<float*>(base + route.plain_bytes) - 2 * he;       // (the tail of the workspace)
    if (in_cache) {
      remap_cache(wide, in_cache, d.num_layers * B, 1, d.hdim, 1, m->user_hdim, m->widen, stream);
      in_cache = wide;
    }
    if (out_cache) { user_h_out = out_cache; out_cache = wide + he; }
  }
  if (route.family == wekws::GRU_PIPE) {
    char* gran = stream_workspace(m, stream, route.granule_bytes, true, unsigned(route.slots) << 8 | unsigned(d.num_layers));
    if (!gran) return WEKWS_HIP_ENOMEM;
    wekws::GruPipeWorkspace ws{};
    ws.ctl = stream_ctl(m, stream, &ws.err);
    if (!ws.ctl) return WEKWS_HIP_ENOMEM;
    ws.seq_in = base;
    ws.seq_top = ws.seq_in + route.seq_bytes;
    ws.sc = reinterpret_cast<float*>(ws.seq_top + route.seq_bytes);
    for (int l = 0; l < d.num_layers; ++l) { ws.gi[l] = gran; gran += route.gi_bytes; }
    for (int l = 0; l + 1 < d.num_layers; ++l) { ws.hs[l] = gran; gran += route.hs_bytes; }
    ws.nf = route.nf_in_kernel ? m->nf_dev : nullptr;
    rc = wekws::launch_gru_pipe(route, m->gq, ws, x, B, T, in_cache, y, out_cache, stream);
  } else if (route.family == wekws::GRU_F16) {
    wekws::GruF16Workspace ws{{base, base + route.seq_bytes}, reinterpret_cast<float*>(base + 2 * route.seq_bytes),
                              reinterpret_cast<float*>(base + 2 * route.seq_bytes + route.gi_bytes)};
    rc = wekws::launch_gru_f16(route, m->gq, ws, x, B, T, in_cache, y, out_cache, stream);
  } else {
    rc = wekws::launch_gru(route, m->gp, x, B, T, in_cache, y, out_cache, stream);
  }
  // (a launcher that refuses what the route chose: the two have drifted apart -- an internal error)
  if (rc == -4) return fail(WEKWS_HIP_EUNSUPPORTED, "internal: %s has no kernel for the route", wekws::gru_family_name(route.family));
  if (rc) return fail(rc, "gru launch failed: %s", hipGetErrorString(hipGetLastError()));
  // streams with a NaN / Inf feature or state (their loads entered the kernels above as 0): the reference's arithmetic
  if (!route.nf_in_kernel) {                               // (the layer-major and exact-f32 kernels: their own launch behind them)
    if (!wekws::launch_gru_nf_fix(m->nf_dev, x, B, T, in_cache, out_cache, y, stream)) return fail(WEKWS_HIP_EDEVICE, "gru non-finite pass: launch failed");
  }
  if (user_h_out) remap_cache(user_h_out, out_cache, d.num_layers * B, 1, m->user_hdim, 1, d.hdim, m->narrow, stream);
  return WEKWS_HIP_OK;
}

// The launcher of the route's family (route.h chose; a launcher refuses -- -4 -- only a route that is not its kernel's)
static int launch_conv_route(const wekws::Route& route, const wekws_hip_model* m, const wekws::CallArgs& a, hipStream_t stream) {
  const wekws_hip_desc& d = m->desc;
  const wekws::StackParams& sp = m->sp;
  const int C = d.hdim;
  switch (route.family) {
    case wekws::ROUTE_DS256_STREAM: return wekws::launch_ds256_stream(route, sp, a, stream);
    case wekws::ROUTE_DS256_G32: return wekws::launch_ds256_g32(route, sp, a, stream);
    case wekws::ROUTE_DS256_MM: return wekws::launch_ds256_mm(route, sp, m->dp.head_a16, a, stream);
    case wekws::ROUTE_DS256_G16: return wekws::launch_ds256_g16(route, sp, a, stream);
    case wekws::ROUTE_DS256_W16: return wekws::launch_ds256_w16(route, sp, a, stream);
    case wekws::ROUTE_DS64_G4: return wekws::launch_ds64_g4(route, sp, a, stream);
    case wekws::ROUTE_MDTC64_STREAM: return wekws::launch_mdtc64_stream(route, sp, a, stream);
    case wekws::ROUTE_MDTC64_G4: case wekws::ROUTE_MDTC32_G4: return wekws::launch_mdtc_g4(route, C, sp, a, stream);
    case wekws::ROUTE_MDTC64_W16: return wekws::launch_mdtc64_w16(route, sp, a, stream);
    case wekws::ROUTE_DENSE_F16: return wekws::launch_dense_stack_f16(route, C, m->dp, a, stream);
    case wekws::ROUTE_CONV_F16: return wekws::launch_conv_stack_f16(route, d.backbone, C, sp, a, stream);
    default: return wekws::launch_conv_stack(route, d.backbone, C, sp, a, stream);
  }
}

// The frames of one conv call, cut into tiles of WEKWS_HIP_TILE_FRAMES that hand the causal context over through ping-pong caches in
// the stream's workspace (route.h: conv_workspace)
static int forward_conv(wekws_hip_model* m, const float* x, int B, int T, const float* in_cache, float* y, float* out_cache,
                        hipStream_t stream) {
  const wekws_hip_desc& d = m->desc;
  const bool per_frame = per_frame_head(d);
  const int TILE = WEKWS_HIP_TILE_FRAMES;
  const int C = d.hdim;
  const wekws::ConvWorkspace w = wekws::conv_workspace(d, m->cache_len, B, T, m->user_hdim != 0);
  const int ntiles = w.ntiles;
  float* ws_cache[2] = {nullptr, nullptr};
  float* gsum = nullptr;
  float* user_out_cache = nullptr;                           // (widened models: where the caller wants the cache)
  if (w.bytes) {
    char* base = stream_workspace(m, stream, w.bytes);
    if (!base) return WEKWS_HIP_ENOMEM;
    auto at = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    if (ntiles > 1) {
      ws_cache[0] = at(w.cache[0]);
      ws_cache[1] = at(w.cache[1]);
      if (w.pooled) gsum = at(w.gsum);
    }
    if (m->user_hdim) {
      // the caller's caches have its own channel count and slice lengths: widened copies (zeros elsewhere) go to the kernels
      if (in_cache) {
        remap_cache(at(w.wide_in), in_cache, B, C, m->cache_len, m->user_hdim, m->user_cache_len, m->widen, stream);
        in_cache = at(w.wide_in);
      }
      if (out_cache) { user_out_cache = out_cache; out_cache = at(w.wide_out); }
    }
  }
  for (int i = 0; i < ntiles; ++i) {
    const int t0 = i * TILE;
    const int Tt = (T - t0 < TILE) ? (T - t0) : TILE;
    wekws::CallArgs a{};
    a.x = x + size_t(t0) * d.idim;
    a.xs_b = int64_t(T) * d.idim;
    a.in_cache = (i == 0) ? in_cache : ws_cache[(i - 1) & 1];
    a.out_cache = (i == ntiles - 1) ? out_cache : ws_cache[i & 1];
    a.y = per_frame ? y + size_t(t0) * d.odim : y;
    a.ys_b = per_frame ? int64_t(T) * d.odim : d.odim;
    a.gsum = gsum;
    a.B = B;
    a.T = Tt;
    a.T_total = T;
    a.first_tile = (i == 0);
    a.last_tile = (i == ntiles - 1);
    a.nf = m->nf_dev;
    // ---- which kernel: one pure function of (shape flags, options, call) -- route.h; tests/test_route.py sweeps it on the CPU
    wekws::RouteCall rcall{};
    rcall.B = B; rcall.T = Tt; rcall.ntiles = ntiles;
    rcall.has_in = a.in_cache != nullptr; rcall.has_out = a.out_cache != nullptr;
    rcall.x16 = reinterpret_cast<uintptr_t>(a.x) % 16 == 0 && a.xs_b % 4 == 0;
    // (the streaming kernels move whole caches with 16-byte accesses: both of the CALL's cache pointers must be 16-byte aligned)
    rcall.cache16 = (reinterpret_cast<uintptr_t>(in_cache) | reinterpret_cast<uintptr_t>(out_cache)) % 16 == 0;
    rcall.cus = m->cus;
    if (ntiles == 1) { rcall.has_in = in_cache != nullptr; rcall.has_out = out_cache != nullptr; }
    const wekws::Route route = wekws::select_conv_route(d, m->rf, m->ro, rcall);
    if (route.family == wekws::ROUTE_NONE) return fail(WEKWS_HIP_EUNSUPPORTED, "no kernel for this call: %s", route.why_not ? route.why_not : "?");
    trace(kTraceConv, route);
    a.head_slices = route.head_slices;
    const int rc = launch_conv_route(route, m, a, stream);
    // (a launcher that refuses what the route chose: the two have drifted apart -- an internal error, never a silent fall-through)
    if (rc == -4)
      return fail(WEKWS_HIP_EUNSUPPORTED, "internal: kernel family %s has no kernel for the route (C=%d nt=%d T=%d cache %d/%d threads %d LDS %d)",
                  wekws::route_family_name(route.family), C, route.nt, Tt, rcall.has_in, rcall.has_out, route.threads, route.lds_bytes);
    if (rc) return fail(rc, "conv-stack launch failed (C=%d nt=%d): %s", C, route.nt, hipGetErrorString(hipGetLastError()));
    if (nf_fix_all()) {                                    // (measurement aid only: the non-finite pass as its own launch)
      if (!launch_conv_nf_fix(a, B, d.idim, C * m->cache_len, stream)) return fail(WEKWS_HIP_EDEVICE, "non-finite pass: launch failed");
    }
  }
  if (user_out_cache) remap_cache(user_out_cache, out_cache, B, m->user_hdim, m->user_cache_len, C, m->cache_len, m->narrow, stream);
  return WEKWS_HIP_OK;
}

// One forward of (B, T) on the model's device, already current: the backbone's path, then the softmax
int forward_call(wekws_hip_model* m, const float* x, int B, int T, const float* in_cache, float* y, float* out_cache, int softmax,
                        hipStream_t stream) {
  const wekws_hip_desc& d = m->desc;
  const bool per_frame = per_frame_head(d);
  int rc;
  if (m->generic) rc = forward_generic(m, x, B, T, in_cache, y, out_cache, stream);
  else if (d.backbone == WEKWS_HIP_BACKBONE_FSMN) rc = forward_fsmn(m, x, B, T, in_cache, y, out_cache, stream);
  else if (d.backbone == WEKWS_HIP_BACKBONE_GRU) rc = forward_gru(m, x, B, T, in_cache, y, out_cache, stream);
  else rc = forward_conv(m, x, B, T, in_cache, y, out_cache, stream);
  if (rc) return rc;
  if (softmax || d.activation == WEKWS_HIP_ACT_SOFTMAX) {
    const int64_t rows = per_frame ? int64_t(B) * T : B;
    const int K = d.odim;
    if (!wekws::launch_softmax_rows(y, rows, K, stream)) return fail(WEKWS_HIP_EDEVICE, "softmax launch failed");
  }
  return WEKWS_HIP_OK;
}

// What a reservation for "calls of up to (B, T)" has to hold: the GRU's scratch is not monotonic in (B, T) (route.h:
// gru_reserve_bytes); every other path's is
static void reserve_need(const wekws_hip_model* m, int B, int T, size_t* plain, size_t* gran) {
  if (!m->generic && m->desc.backbone == WEKWS_HIP_BACKBONE_GRU)
    return wekws::gru_reserve_bytes(m->desc, m->ro, wekws::GruCall{B, T, 1, m->user_hdim != 0, m->cus}, plain, gran);
  *plain = workspace_need(m, B, T);
  *gran = 0;
}


extern "C" {

size_t wekws_hip_workspace_bytes(const wekws_hip_model* m, int B, int T) { return m ? workspace_need(m, B, T) + granule_need(m, B, T) : 0; }


int wekws_hip_reserve(wekws_hip_model* m, int B, int T, void* stream_) {
  if (!m) return fail(WEKWS_HIP_EINVAL, "NULL model");
  size_t need = 0, gran = 0;
  reserve_need(m, B, T, &need, &gran);
  if (!need && !gran) return WEKWS_HIP_OK;
  DeviceGuard guard(m->device);
  if (!guard.ok) return fail(WEKWS_HIP_EDEVICE, "hipSetDevice(%d)", m->device);
  if (need && !stream_workspace(m, static_cast<hipStream_t>(stream_), need)) return WEKWS_HIP_ENOMEM;
  if (gran && !stream_workspace(m, static_cast<hipStream_t>(stream_), gran, true)) return WEKWS_HIP_ENOMEM;
  if (m->desc.backbone == WEKWS_HIP_BACKBONE_GRU && m->ro.gru_pipe && !stream_ctl(m, static_cast<hipStream_t>(stream_))) return WEKWS_HIP_ENOMEM;
  return WEKWS_HIP_OK;
}

int wekws_hip_forward_status(wekws_hip_model* m, void* stream_) {
  if (!m) return fail(WEKWS_HIP_EINVAL, "NULL model");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DeviceGuard guard(m->device);
  if (!guard.ok) return fail(WEKWS_HIP_EDEVICE, "hipSetDevice(%d)", m->device);
  // the documented contract, for EVERY model: the stream is synchronised when this returns (the C++ runtime's Forward reads
  // its host buffer behind it) -- then the health word, which only streams with wavefront launches have
  const hipError_t e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "hipStreamSynchronize: %s", hipGetErrorString(e));
  return stream_health(m, stream);
}

int wekws_hip_forward(wekws_hip_model* m, const float* x, int B, int T, const float* in_cache, float* y,
                      float* out_cache, int softmax, void* stream_) {
  if (!m || !x || !y) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (B < 0 || T <= 0) return fail(WEKWS_HIP_EINVAL, "B=%d T=%d", B, T);
  if (B == 0) return WEKWS_HIP_OK;
  if (in_cache && in_cache == out_cache) return fail(WEKWS_HIP_EINVAL, "in_cache and out_cache must not alias");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  // the kernels go to the model's device whatever the calling thread's current device is (a default stream, NULL, means
  // that device's default stream); the caller's device is current again on return
  DeviceGuard guard(m->device);
  if (!guard.ok) return fail(WEKWS_HIP_EDEVICE, "hipSetDevice(%d)", m->device);
  trace_reset(m->generic ? kTraceAnyShape : kTraceOther);
  return forward_call(m, x, B, T, in_cache, y, out_cache, softmax, stream);
}

}  // extern "C"
