// Where a forward reports the route of every launch (model.h: trace_reset, trace) -- the one unit that differs between the two libraries.
// libwekws_hip.so: the sinks are empty, the unit exports nothing and holds no kernel.  libwekws_hip_hooks.so (make hooks: this unit
// compiled with -DWEKWS_TEST_HOOKS, every other object shared with the product library): the sinks record, and the unit carries the test
// hooks: the route trace of a forward, the routing functions of route.h and the blob layout of blob_layout.h without a device, the GRU
// epoch, a CU hog, the fbank's plan and table, the row softmax on chosen logits, the resampler's taps and plan (a rate bank's too, and the check of a bank call's rows, wire bytes included; the stream planner of both handles through a script of calls), the CTC decoder's keyword-set table.  Not part of the ABI in include/wekws_hip.h.
#include <algorithm>
#include <cstring>
#include <vector>

#include "model.h"
#include "ds256_stream.hip.h"
#include "mdtc64_stream.hip.h"
#include "ctc_kws_sets.h"
#include "resample.hip.h"
#include "resample_bank.hip.h"

#ifndef WEKWS_TEST_HOOKS
void trace_reset(int) {}
void trace(int, const wekws::Route&) {}
void trace(int, const wekws::GruRoute&) {}
void trace(int, const wekws::FsmnRoute&) {}
#else
static thread_local wekws::Route g_last_route{};             // the route of this thread's last conv launch
// the route of EVERY tile of this thread's last forward (wekws_hip_debug_route_trace), as records of 9 ints
struct RouteTrace {
  int path = kTraceOther, ntiles = 0;
  int rec[kTraceMaxTiles][kRecInts];
};
static thread_local RouteTrace g_route_trace;
// family, nt, split, ctx, fast, grid, threads, lds, utts_per_wg
static void route_record(const wekws::Route& r, int* o) {
  const int v[kRecInts] = {r.family, r.nt, r.split, r.ctx, r.fast, r.grid, r.threads, r.lds_bytes, r.utts_per_wg};
  for (int i = 0; i < kRecInts; ++i) o[i] = v[i];
}
// family, nn, spw, tchunk (0: one launch), nchunks, slots, tiles, grid, pk | k2 << 1 | nf_in_kernel << 2
static void route_record(const wekws::GruRoute& r, int* o) {
  const int v[kRecInts] = {r.family, r.nn, r.spw, r.chunked ? r.tchunk : 0, r.nchunks, r.slots, r.tiles, r.grid,
                           r.pk | r.k2 << 1 | r.nf_in_kernel << 2};
  for (int i = 0; i < kRecInts; ++i) o[i] = v[i];
}
// tile_frames, nt, u, head_slices, grid, lds, ntiles, 0, 0
static void route_record(const wekws::FsmnRoute& r, int* o) {
  const int v[kRecInts] = {r.tile_frames, r.nt, r.u, r.head_slices, r.grid, r.lds_bytes, r.ntiles, 0, 0};
  for (int i = 0; i < kRecInts; ++i) o[i] = v[i];
}
template <class R>
static void trace_record(int path, const R& r) {
  g_route_trace.path = path;
  if (g_route_trace.ntiles < kTraceMaxTiles) route_record(r, g_route_trace.rec[g_route_trace.ntiles]);
  ++g_route_trace.ntiles;
}
void trace(int path, const wekws::Route& r) { g_last_route = r; trace_record(path, r); }
void trace(int path, const wekws::GruRoute& r) { trace_record(path, r); }
void trace(int path, const wekws::FsmnRoute& r) { trace_record(path, r); }
void trace_reset(int path) {
  g_route_trace.path = path;
  g_route_trace.ntiles = 0;
}
// the reason text of a debug entry point
static void say(char* why, int why_len, const char* t) {
  if (why && why_len > 0 && t) { std::strncpy(why, t, size_t(why_len) - 1); why[why_len - 1] = 0; }
}

// Set the launch epoch of the stream's wavefront control block, so that a test can walk the 32-bit tag counter across its wrap
// (tests/test_hip_parity.py::test_gru_wavefront_epoch_wrap).
extern "C" int wekws_hip_debug_set_gru_epoch(wekws_hip_model* m, void* stream_, unsigned epoch) {
  if (!m) return fail(WEKWS_HIP_EINVAL, "NULL model");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DeviceGuard guard(m->device);
  if (!guard.ok) return fail(WEKWS_HIP_EDEVICE, "hipSetDevice(%d)", m->device);
  unsigned* ctl = stream_ctl(m, stream);
  if (!ctl) return WEKWS_HIP_ENOMEM;
  if (hipMemcpyAsync(ctl, &epoch, sizeof(epoch), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return fail(WEKWS_HIP_EDEVICE, "setting the epoch: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}
// A tenant that keeps CUs busy: `blocks` workgroups of 128 KB of LDS each (one per CU, like the wavefront's own), every one
// holding its CU for `ms` milliseconds of wall clock.  tests: a wavefront launch whose later workgroups find no CU for longer
// than its bounded waits must END (not hang) and be reported by the next call; a shorter squeeze must change nothing.
// ms < 0: the same occupancy with every SIMD BUSY (matrix + vector instructions, no memory traffic) for -ms milliseconds -- to
// tell a neighbour's compute / power from a neighbour's memory traffic (tools/probe/gru_neighbours.py)
extern "C" __global__ void debug_hog_kernel(unsigned long long ticks, int busy) {
  extern __shared__ char hog_lds[];
  if (threadIdx.x == 0) hog_lds[0] = 1;
  const unsigned long long t0 = wall_clock64();              // 100 MHz
  if (!busy) {
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
    return;
  }
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  typedef float f4 __attribute__((ext_vector_type(4)));
  h8 a = {1, 1, 1, 1, 1, 1, 1, 1}, b = a;
  f4 c0 = {0, 0, 0, 0}, c1 = c0;
  float v = float(threadIdx.x);
  while (wall_clock64() - t0 < ticks) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c1, 0, 0, 0);
      v = fmaf(v, 1.0001f, 0.5f);
    }
  }
  if (c0[0] + c1[0] + v == 12345.f) hog_lds[1] = 1;
}
// The routing functions of route.h, callable WITHOUT a device (tests/test_route.py, hooks library only).
//   desc: any conv descriptor wekws_hip_create accepts.  opts[9] (or NULL = the defaults for that precision): w16_ok, g16_ok, g16_ctx,
//   g16_one_pass, stream_ok, mdtc16_ok, mm_ok (-1: the default: CTC-sized heads), f32, split.  call[8]: B, T (of the tile), ntiles,
//   has_in, has_out, x16, cache16, cus.  out[16]: plan kind, built C, built ks, family, nt, split, ctx, fast, grid, threads, lds,
//   utts_per_wg, cache_len (built shape), max_pad, head_slices, effective precision (of the model under these options).  why: the
//   reason text for "any-shape path" / "no kernel".  Returns 0.
extern "C" int wekws_hip_debug_conv_route(const wekws_hip_desc* desc, const int* opts, const int* call, int* out, char* why, int why_len) {
  if (!desc || !call || !out || !desc_conv(*desc)) return WEKWS_HIP_EINVAL;
  for (int i = 0; i < 16; ++i) out[i] = 0;
  if (why && why_len > 0) why[0] = 0;
  const wekws::ShapePlan plan = wekws::conv_shape_plan(*desc, wekws::kAmaxMaxBlocks);
  out[0] = plan.kind; out[1] = plan.C; out[2] = plan.ks;
  if (plan.kind == wekws::SHAPE_GENERIC) { say(why, why_len, plan.why); return WEKWS_HIP_OK; }
  wekws_hip_desc d = *desc;
  d.hdim = plan.C; d.kernel_size = plan.ks;
  const int cache_len = wekws::conv_route_flags(d, 0, 0).cache_len;
  const wekws::RouteFlags ff = wekws::conv_route_flags(d, int(wekws::ds256_stream_lds_bytes(cache_len)), int(wekws::mdtc64_stream_lds_bytes(cache_len)));
  wekws::RouteOptions o = wekws::route_defaults(d, ff);
  if (opts) {
    o.w16_ok = opts[0]; o.g16_ok = opts[1]; o.g16_ctx = opts[2]; o.g16_one_pass = opts[3]; o.stream_ok = opts[4];
    wekws::apply_route_option(o, d, ff, WEKWS_HIP_OPT_MDTC16, opts[5]);
    wekws::apply_route_option(o, d, ff, WEKWS_HIP_OPT_MM, opts[6]);
    o.f32 = opts[7]; o.split = opts[8];
  }
  wekws::RouteCall c{call[0], call[1], call[2], call[3], call[4], call[5], call[6], call[7]};
  const wekws::Route r = wekws::select_conv_route(d, ff, o, c);
  out[3] = r.family; out[4] = r.nt; out[5] = r.split; out[6] = r.ctx; out[7] = r.fast; out[8] = r.grid; out[9] = r.threads; out[10] = r.lds_bytes;
  out[11] = r.utts_per_wg; out[12] = ff.cache_len; out[13] = ff.max_pad; out[14] = r.head_slices;
  out[15] = wekws::effective_precision(d, ff, o, c.cus);
  if (r.family == wekws::ROUTE_NONE) say(why, why_len, r.why_not);
  else say(why, why_len, wekws::route_family_name(r.family));
  return WEKWS_HIP_OK;
}
// the route of the calling thread's last conv launch: out[9] = family, nt, split, ctx, fast, grid, threads, lds, utts_per_wg
extern "C" int wekws_hip_debug_last_route(int* out) {
  if (!out) return WEKWS_HIP_EINVAL;
  route_record(g_last_route, out);
  return WEKWS_HIP_OK;
}
// GRU (hooks library only): desc: any GRU descriptor wekws_hip_create accepts; opts: nopts (WEKWS_HIP_OPT_*, value) pairs applied to
// the defaults.  call[5]: B, T, x16, cus, with_reserve.  out[20] (int64): plan kind, built hidden size, the 9 ints of the trace
// record (route_record), stages, slots_p, lds, chunked, plain bytes, granule bytes, reserved plain / granule bytes (with_reserve),
// effective precision.  why: the family's name, or the reason.  Returns 0.
extern "C" int wekws_hip_debug_gru_route(const wekws_hip_desc* desc, const int* opts, int nopts, const int* call, int64_t* out, char* why,
                                         int why_len) {
  if (!desc || !call || !out || desc->backbone != WEKWS_HIP_BACKBONE_GRU || (nopts && !opts)) return WEKWS_HIP_EINVAL;
  for (int i = 0; i < 20; ++i) out[i] = 0;
  const wekws::ShapePlan plan = wekws::gru_shape_plan(*desc);
  out[0] = plan.kind; out[1] = plan.C;
  if (plan.kind == wekws::SHAPE_GENERIC) { say(why, why_len, plan.why); return WEKWS_HIP_OK; }
  wekws_hip_desc d = *desc;
  d.hdim = plan.C;
  const wekws::RouteFlags f{};
  wekws::RouteOptions o = wekws::route_defaults(d, f);
  for (int i = 0; i < nopts; ++i)
    if (wekws::apply_route_option(o, d, f, opts[2 * i], opts[2 * i + 1])) return WEKWS_HIP_EINVAL;
  const wekws::GruCall c{call[0], call[1], call[2], plan.kind == wekws::SHAPE_PADDED, call[3]};
  const wekws::GruRoute r = wekws::select_gru_route(d, o, c);
  int rec[kRecInts];
  route_record(r, rec);
  for (int i = 0; i < kRecInts; ++i) out[2 + i] = rec[i];
  out[11] = r.stages; out[12] = r.slots_p; out[13] = r.lds_bytes; out[14] = r.chunked;
  out[15] = int64_t(r.plain_bytes); out[16] = int64_t(r.granule_bytes);
  if (call[4]) {
    size_t p = 0, g = 0;
    wekws::gru_reserve_bytes(d, o, c, &p, &g);
    out[17] = int64_t(p); out[18] = int64_t(g);
  }
  out[19] = wekws::effective_precision(d, f, o, c.cus);
  say(why, why_len, r.family == wekws::GRU_NONE ? r.why_not : wekws::gru_family_name(r.family));
  return WEKWS_HIP_OK;
}
// FSMN (hooks library only): desc: any FSMN descriptor; opts / nopts as above.  call[4]: B, T, tile index, cus.  out[16]: plan kind,
// max_nt, the 9 ints of the tile's trace record, workspace bytes of the call, effective precision, 0...  Returns 0.
extern "C" int wekws_hip_debug_fsmn_route(const wekws_hip_desc* desc, const int* opts, int nopts, const int* call, int64_t* out, char* why,
                                          int why_len) {
  if (!desc || !call || !out || desc->backbone != WEKWS_HIP_BACKBONE_FSMN || (nopts && !opts)) return WEKWS_HIP_EINVAL;
  for (int i = 0; i < 16; ++i) out[i] = 0;
  const wekws::FsmnPlan plan = wekws::fsmn_shape_plan(*desc);
  out[0] = plan.kind; out[1] = plan.max_nt;
  if (plan.kind == wekws::SHAPE_GENERIC) { say(why, why_len, plan.why); return WEKWS_HIP_OK; }
  const wekws::RouteFlags f{};
  wekws::RouteOptions o = wekws::route_defaults(*desc, f);
  for (int i = 0; i < nopts; ++i)
    if (wekws::apply_route_option(o, *desc, f, opts[2 * i], opts[2 * i + 1])) return WEKWS_HIP_EINVAL;
  const wekws::FsmnRoute r = wekws::select_fsmn_route(plan, *desc, o, call[0], call[1], call[2], call[3]);
  int rec[kRecInts];
  route_record(r, rec);
  for (int i = 0; i < kRecInts; ++i) out[2 + i] = rec[i];
  out[11] = int64_t(r.ws_bytes);
  out[12] = wekws::effective_precision(*desc, f, o, call[3]);
  say(why, why_len, r.why_not ? r.why_not : "fsmn_f16");
  return WEKWS_HIP_OK;
}
// The plan of a wekws_hip_forward_streams call (route.h: plan_streams), WITHOUT a device (hooks library only): desc: any descriptor
// wekws_hip_create accepts; opts / nopts as above; call[3]: B, Tcap, cus; frames[B].  out[16]: kind (0 grouped, 1 ds256_stream, 2
// fsmn_f16), live rows, largest frame count, groups, rows a group holds at most (0: any number), then conv family, split, grid, LDS
// bytes (kind 1), then nt, u, head slices, grid, LDS bytes (kind 2), 0, 0.  order[B]: the live rows in launch order; group_start[B + 1]:
// ngroups + 1 offsets into order; group_T[B]: the frame count of every group.  why: the reason of a grouped plan.  Returns 0.
extern "C" int wekws_hip_debug_streams_plan(const wekws_hip_desc* desc, const int* opts, int nopts, const int* call, const int32_t* frames,
                                            int* out, int32_t* order, int32_t* group_start, int32_t* group_T, char* why, int why_len) {
  if (!desc || !call || !frames || !out || !order || !group_start || !group_T || (nopts && !opts) || call[0] < 0 || !blob_elems(*desc))
    return WEKWS_HIP_EINVAL;
  for (int i = 0; i < 16; ++i) out[i] = 0;
  if (why && why_len > 0) why[0] = 0;
  wekws_hip_desc d = *desc;
  wekws::RouteFlags f{};
  wekws::FsmnPlan fp{};
  bool plain = false;
  if (desc_conv(d)) {
    const wekws::ShapePlan sp = wekws::conv_shape_plan(d, wekws::kAmaxMaxBlocks);
    plain = sp.kind == wekws::SHAPE_AS_IS;
    if (sp.kind != wekws::SHAPE_GENERIC) {
      d.hdim = sp.C; d.kernel_size = sp.ks;
      const int cache_len = wekws::conv_route_flags(d, 0, 0).cache_len;
      f = wekws::conv_route_flags(d, int(wekws::ds256_stream_lds_bytes(cache_len)), int(wekws::mdtc64_stream_lds_bytes(cache_len)));
    }
  } else if (d.backbone == WEKWS_HIP_BACKBONE_FSMN) {
    fp = wekws::fsmn_shape_plan(d);
    plain = fp.kind == wekws::SHAPE_AS_IS;
  } else {
    plain = wekws::gru_shape_plan(d).kind == wekws::SHAPE_AS_IS;
  }
  wekws::RouteOptions o = wekws::route_defaults(d, f);
  for (int i = 0; i < nopts; ++i)
    if (wekws::apply_route_option(o, d, f, opts[2 * i], opts[2 * i + 1])) return WEKWS_HIP_EINVAL;
  const wekws::StreamsPlan p = wekws::plan_streams(d, f, o, fp, plain, call[2], call[0], call[1], frames, order, group_start, group_T);
  const int v[16] = {p.kind, p.live, p.max_T, p.ngroups, p.slots, p.conv.family, p.conv.split, p.conv.grid, p.conv.lds_bytes,
                     p.fsmn.nt, p.fsmn.u, p.fsmn.head_slices, p.fsmn.grid, p.fsmn.lds_bytes, 0, 0};
  for (int i = 0; i < 16; ++i) out[i] = v[i];
  say(why, why_len, p.why);
  return WEKWS_HIP_OK;
}
// The weight blob's layout (blob_layout.h), WITHOUT a device (tests/test_blob_layout.py, hooks library only): desc: any descriptor
// wekws_hip_blob_elems accepts.  out (int64, 4 per tensor): offset in floats, rows, cols, inner of every tensor in blob order, at most
// max_tensors of them.  Returns the number of tensors of the blob, or WEKWS_HIP_EINVAL.
extern "C" int wekws_hip_debug_blob_layout(const wekws_hip_desc* desc, int64_t* out, int max_tensors) {
  if (!desc || !blob_elems(*desc) || (max_tensors > 0 && !out)) return WEKWS_HIP_EINVAL;
  int n = 0;
  wekws::for_each_tensor(wekws::blob_layout(*desc), [&](const wekws::BlobTensor& t) {
    if (n < max_tensors) { out[4 * n] = t.off; out[4 * n + 1] = t.rows; out[4 * n + 2] = t.cols; out[4 * n + 3] = t.inner; }
    ++n;
  });
  return n;
}
// ... and one tensor BY NAME, through the accessor the library's own code reads it with: `name` of block / layer `unit` (ignored
// outside the units).  out[4] as above; a tensor the model does not have has rows = 0.  Returns 0, or WEKWS_HIP_EINVAL (unknown name).
extern "C" int wekws_hip_debug_blob_tensor(const wekws_hip_desc* desc, const char* name, int unit, int64_t* out) {
  if (!desc || !name || !out || !blob_elems(*desc)) return WEKWS_HIP_EINVAL;
  const wekws::BlobLayout L = wekws::blob_layout(*desc);
  const wekws::ConvWeights c = L.block(unit);
  const wekws::GruWeights g = L.gru_layer(unit);
  const wekws::FsmnWeights f = L.fsmn_layer(unit);
  const struct { const char* name; wekws::BlobTensor t; } table[] = {
      {"pre_w", L.pre_w()}, {"pre_b", L.pre_b()}, {"in1_w", L.in1_w()}, {"in1_b", L.in1_b()}, {"in2_w", L.in2_w()}, {"in2_b", L.in2_b()},
      {"wd", c.wd}, {"bd", c.bd}, {"w1", c.w1}, {"b1", c.b1}, {"w2", c.w2}, {"b2", c.b2},
      {"w_ih", g.w_ih}, {"w_hh", g.w_hh}, {"b_ih", g.b_ih}, {"b_hh", g.b_hh},
      {"wproj", f.wproj}, {"taps", f.taps}, {"waff", f.waff}, {"baff", f.baff},
      {"head_w", L.head_w()}, {"head_b", L.head_b()}, {"head_w2", L.head_w2()}, {"head_b2", L.head_b2()},
      {"out1_w", L.out1_w()}, {"out1_b", L.out1_b()}, {"out2_w", L.out2_w()}, {"out2_b", L.out2_b()}};
  for (const auto& e : table)
    if (!std::strcmp(name, e.name)) {
      out[0] = e.t.off; out[1] = e.t.rows; out[2] = e.t.cols; out[3] = e.t.inner;
      return WEKWS_HIP_OK;
    }
  return WEKWS_HIP_EINVAL;
}
// the route of every tile of the calling thread's last forward: out[0] = path (0: no forward yet; 1: the conv routes of route.h;
// 2: the any-shape path of generic.hip.h; 3: the GRU route of route.h -- one record; 4: the FSMN routes of route.h), out[1] =
// records of the call, then per record (at most max_tiles, and the first 256 of a call) its 9 ints: conv, the values of
// wekws_hip_debug_last_route; GRU / FSMN, route_record's.  out holds 2 + 9 * max_tiles ints.  Returns the number of records written.
extern "C" int wekws_hip_debug_route_trace(int* out, int max_tiles) {
  if (!out || max_tiles < 0) return WEKWS_HIP_EINVAL;
  const RouteTrace& t = g_route_trace;
  out[0] = t.path; out[1] = t.ntiles;
  int n = t.ntiles < kTraceMaxTiles ? t.ntiles : kTraceMaxTiles;
  n = n < max_tiles ? n : max_tiles;
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < kRecInts; ++k) out[2 + kRecInts * i + k] = t.rec[i][k];
  return n;
}
extern "C" int wekws_hip_debug_hog(int device, int blocks, int ms, void* stream_) {
  DeviceGuard guard(device);
  const int busy = ms < 0;
  if (busy) ms = -ms;
  if (!guard.ok || blocks <= 0 || ms > 2000) return fail(WEKWS_HIP_EINVAL, "hog: device %d blocks %d ms %d", device, blocks, ms);
  static wekws::DynLdsGrant grant;
  if (wekws::grant_dynamic_lds(debug_hog_kernel, 128 * 1024, grant)) return fail(WEKWS_HIP_EDEVICE, "hog: LDS grant");
  hipLaunchKernelGGL(debug_hog_kernel, dim3(blocks), dim3(busy ? 512 : 64), 128 * 1024, static_cast<hipStream_t>(stream_), 100000ull * ms, busy);
  return hipGetLastError() == hipSuccess ? WEKWS_HIP_OK : fail(WEKWS_HIP_EDEVICE, "hog launch");
}

// --------------------------------------------- fbank ---------------------------------------------
// what the last fbank launch of this thread ran, the table plan, the device table
// out[8]: rounds, sample size in bytes, pair_ok, grid, resident, B, nsamp, nframes as launch_fbank recorded them at this thread's last launch
extern "C" int wekws_hip_debug_fbank_last(int* out) {
  if (!out) return WEKWS_HIP_EINVAL;
  for (int i = 0; i < 8; ++i) out[i] = wekws::fbank_last_launch()[i];
  return WEKWS_HIP_OK;
}
// The table plan of a configuration, WITHOUT a device (fbank_build_tables alone).  out[16]: rounds (mel slots per lane), nslots, spectrum
// stride (512 / the reference's transform length), slots of the widest filter, kFbankFW, kFbankWaves, mel_first_off, mel_size_off,
// mel_start_off, mel_w_off, mel_w_count, slot_first_off, slot_bin_off, slot_w_off, table_floats, first empty filter (-1: none; then
// the plan before it is not filled in and wekws_hip_fbank_create refuses the configuration).
extern "C" int wekws_hip_debug_fbank_plan(const wekws_hip_fbank_cfg* cfg, int* out) {
  if (!cfg || !out || cfg->num_bins <= 0 || cfg->num_bins > wekws::kFbankMaxBins || cfg->sample_rate <= 0 || cfg->frame_length <= 64 ||
      cfg->frame_length > wekws::kFbankMaxFft || cfg->frame_shift <= 0)
    return WEKWS_HIP_EINVAL;
  for (int i = 0; i < 16; ++i) out[i] = 0;
  wekws::FbankParams fp{};
  std::vector<float> t;
  out[15] = wekws::fbank_build_tables(cfg->num_bins, cfg->sample_rate, cfg->frame_length, cfg->frame_shift, cfg->window, &fp, &t);
  out[2] = wekws::kFbankMaxFft / wekws::fbank_ref_points(cfg->frame_length);
  out[4] = wekws::kFbankFW;
  out[5] = wekws::kFbankWaves;
  if (out[15] >= 0) return WEKWS_HIP_OK;
  int widest = 0;
  for (int b = 0; b < fp.num_bins; ++b) widest = std::max(widest, (int(t[size_t(fp.mel_size_off) + b]) + 15) / 16);
  const int v[15] = {(fp.nslots + 63) / 64, fp.nslots, out[2], widest, out[4], out[5], fp.mel_first_off, fp.mel_size_off, fp.mel_start_off,
                     fp.mel_w_off, fp.mel_w_count, fp.slot_first_off, fp.slot_bin_off, fp.slot_w_off, fp.table_floats};
  for (int i = 0; i < 15; ++i) out[i] = v[i];
  return WEKWS_HIP_OK;
}
// Read (set == 0) or overwrite (set != 0) the handle's device table: n must be its table_floats.  The kernel takes its per-lane constants
// (twiddles, window, mel slots) from this table at every launch, so a test can run it on a perturbed table and put the table back.
extern "C" int wekws_hip_debug_fbank_tables(wekws_hip_fbank* f, float* host_buf, int n, int set) {
  if (!f || !host_buf || n != f->fp.table_floats) return fail(WEKWS_HIP_EINVAL, "fbank tables: n=%d, the table has %d floats", n, f ? f->fp.table_floats : 0);
  DeviceGuard guard(f->device);
  if (!guard.ok) return fail(WEKWS_HIP_EDEVICE, "hipSetDevice(%d)", f->device);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess)
    e = set ? hipMemcpy(f->d_tables, host_buf, size_t(n) * sizeof(float), hipMemcpyHostToDevice)
            : hipMemcpy(host_buf, f->d_tables, size_t(n) * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "fbank tables: %s", hipGetErrorString(e));
  return WEKWS_HIP_OK;
}

// --------------------------------------------- softmax ---------------------------------------------
// softmax_rows_kernel in place on y (rows, K), through the launch statement wekws_hip_forward uses for forward_softmax: a test
// reaches the kernel with logits of its choice (tests/test_hip_softmax_f64.py) instead of the ones a model happens to produce.
extern "C" int wekws_hip_debug_softmax_rows(float* y, int64_t rows, int K, void* stream_) {
  if (!y || rows < 0 || K <= 0 || (rows + 3) / 4 > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "softmax_rows: rows=%lld K=%d", (long long)rows, K);
  if (rows == 0) return WEKWS_HIP_OK;
  if (!wekws::launch_softmax_rows(y, rows, K, static_cast<hipStream_t>(stream_))) return fail(WEKWS_HIP_EDEVICE, "softmax launch failed");
  return WEKWS_HIP_OK;
}

// --------------------------------------------- resample ---------------------------------------------
// The plan of a rate pair, WITHOUT a device (resample_plan.h alone).  dims[10]: o, n, width, K, most live taps of a phase, stride of
// the live table, LDS bytes of a launch, samples of the input tile, history capacity of a stream, outputs of a tile.  taps: NULL, or
// (n, K) floats; first / last: NULL, or (n) ints -- filled only if cap_taps >= n K and cap_phases >= n.  Returns 0, WEKWS_HIP_EINVAL
// for parameters no resampler has.  (A pair the kernels refuse for its size still has a plan; taps are then only computed on request.)
extern "C" int wekws_hip_debug_resample_plan(int orig, int neu, int lpw, double rolloff, int64_t* dims, float* taps, int64_t cap_taps,
                                             int32_t* first, int32_t* last, int64_t cap_phases) {
  if (!dims) return WEKWS_HIP_EINVAL;
  wekws::ResamplePlan p;
  if (wekws::resample_plan_ranges(orig, neu, lpw, rolloff, &p)) return WEKWS_HIP_EINVAL;
  const int64_t v[10] = {p.o, p.n, p.width, p.K, p.max_live, wekws::resample_stride(p.max_live), wekws::resample_lds_bytes(p),
                         wekws::resample_tile_cap(p), (wekws::resample_hist_cap(p) + 1) & ~1, wekws::kResampleTile};
  for (int i = 0; i < 10; ++i) dims[i] = v[i];
  if (first && last && cap_phases >= p.n)
    for (int i = 0; i < p.n; ++i) { first[i] = p.first[size_t(i)]; last[i] = p.last[size_t(i)]; }
  if (taps && cap_taps >= int64_t(p.n) * p.K) {
    wekws::resample_plan_taps(&p);
    std::memcpy(taps, p.taps.data(), p.taps.size() * sizeof(float));
  }
  return WEKWS_HIP_OK;
}
// One push onto one stream, WITHOUT a device: the function wekws_hip_resample_push decides every row with.  A stream that has received
// N samples is given nsamp more (flush: and ended).  out[4]: outputs emitted in total after the push, first sample the stream keeps,
// outputs emitted in total BEFORE it (resample_emit_count(N)), capacity wekws_hip_resample_max_out gives for nsamp.  Returns 0.
extern "C" int wekws_hip_debug_resample_step(int orig, int neu, int lpw, double rolloff, int64_t N, int64_t nsamp, int flush, int64_t* out) {
  if (!out || N < 0 || nsamp < 0) return WEKWS_HIP_EINVAL;
  wekws::ResamplePlan p;
  if (wekws::resample_plan_ranges(orig, neu, lpw, rolloff, &p)) return WEKWS_HIP_EINVAL;
  const wekws::ResampleStep s = wekws::resample_step(p, N, nsamp, flush);
  out[0] = s.total; out[1] = s.keep_from; out[2] = wekws::resample_emit_count(p, N); out[3] = wekws::resample_max_out(p, nsamp, flush);
  return WEKWS_HIP_OK;
}
// A whole schedule of pushes onto one stream (the last one flushed if flush_last), WITHOUT a device: totals[k] / keeps[k] after push k.
extern "C" int wekws_hip_debug_resample_schedule(int orig, int neu, int lpw, double rolloff, const int32_t* chunks, int nchunks,
                                                 int flush_last, int64_t* totals, int64_t* keeps) {
  if (!chunks || !totals || !keeps || nchunks < 0) return WEKWS_HIP_EINVAL;
  wekws::ResamplePlan p;
  if (wekws::resample_plan_ranges(orig, neu, lpw, rolloff, &p)) return WEKWS_HIP_EINVAL;
  int64_t N = 0;
  for (int k = 0; k < nchunks; ++k) {
    if (chunks[k] < 0) return WEKWS_HIP_EINVAL;
    const wekws::ResampleStep s = wekws::resample_step(p, N, chunks[k], flush_last && k == nchunks - 1);
    N += chunks[k];
    totals[k] = s.total; keeps[k] = s.keep_from;
  }
  return WEKWS_HIP_OK;
}
// Round the taps of one member of the handle -- its live table and its full one -- to fp16 values, in place: the negative control of
// the resampler's bar (a kernel that took its taps at half precision must miss it).  There is no way back: destroy the handle afterwards.
static int resample_round_taps_f16(wekws_hip_resample* r, int member) {
  if (!r) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  if (member < 0 || member >= int(r->P.size())) return fail(WEKWS_HIP_EINVAL, "member %d outside 0..%d", member, int(r->P.size()) - 1);
  DeviceGuard guard(r->device);
  if (!guard.ok) return fail(WEKWS_HIP_EDEVICE, "hipSetDevice(%d)", r->device);
  const wekws::ResampleParams& P = r->P[size_t(member)];
  float* const d_live = r->d_live[size_t(member)];
  float* const d_full = r->d_full[size_t(member)];
  std::vector<float> live(size_t(P.n) * P.stride), full(size_t(P.n) * P.K);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(live.data(), d_live, live.size() * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(full.data(), d_full, full.size() * sizeof(float), hipMemcpyDeviceToHost);
  for (float& v : live) v = float(_Float16(v));
  for (float& v : full) v = float(_Float16(v));
  if (e == hipSuccess) e = hipMemcpy(d_live, live.data(), live.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_full, full.data(), full.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "%s taps: %s", r->name(), hipGetErrorString(e));
  return WEKWS_HIP_OK;
}
extern "C" int wekws_hip_debug_resample_round_taps_f16(wekws_hip_resample* r) { return resample_round_taps_f16(r, 0); }
extern "C" int wekws_hip_debug_resample_bank_round_taps_f16(wekws_hip_resample* r, int member) { return resample_round_taps_f16(r, member); }

// The stream planner of both handles (resample_streams.h), WITHOUT a device, through a script of calls on max_streams streams of a
// bank of (rates, encs) pairs (encs NULL: every member s16).  single: planned as the single-rate handle plans (num must be 1).
// script: n_ints int32, one call after the other:
//   0, wire_call, B, width, flush, mcap, ids[B], nsamp[B]   a push (pcm at address 0), committed if it is accepted
//   1, n, ids[n]                                            reset
//   2, member, n, ids[n]                                    set_rate
// Per call k < max_calls: outcome[4 k ..]: the refusal (ResampleStreamsRefusal; reset / set_rate: 1 for an id outside, else 0), the
// row or index it is about (-1: none), the rows' refusal (ResampleBankRowRefusal), the most outputs of a row (of a call planned to its end);
// rows (max_calls, max_streams, 12): the table of an accepted push as it is uploaded, in slot order; counts (max_calls, max_streams, 4):
// wekws_hip_resample_counts of every stream after the call.  Returns the number of calls, or a negative code for a bank no resampler
// has, a malformed script or more calls than max_calls.
extern "C" int wekws_hip_debug_resample_streams_script(const int32_t* rates, const int32_t* encs, int num, int neu, int lpw, double rolloff,
                                                       int single, int max_streams, int max_chunk, const int32_t* script, int n_ints,
                                                       int max_calls, int64_t* outcome, int32_t* rows, int64_t* counts) {
  static_assert(sizeof(wekws::ResampleRow) == 12 * sizeof(int32_t), "rows are 12 ints");
  if (!script || !outcome || !rows || !counts || max_streams < 1 || max_chunk < 1 || (single && num != 1)) return WEKWS_HIP_EINVAL;
  wekws::ResampleBankPlan bp;
  int bad = -1;
  const wekws::ResampleBankRefusal r = wekws::resample_bank_plan(rates, encs, num, neu, lpw, rolloff, &bp, &bad);
  if (r == wekws::kResampleBankLds) return WEKWS_HIP_EUNSUPPORTED;
  if (r != wekws::kResampleBankOk) return WEKWS_HIP_EINVAL;
  wekws::ResampleStreams S;
  wekws::resample_streams_init(&S, max_streams, max_chunk, wekws::resample_bank_hist_cap(bp), single != 0);
  std::vector<int32_t> yields(max_streams, 0);
  int k = 0;
  for (int at = 0; at < n_ints; ++k) {
    if (k >= max_calls) return WEKWS_HIP_EINVAL;
    int64_t* const res = outcome + 4 * int64_t(k);
    res[0] = 0; res[1] = -1; res[2] = 0; res[3] = 0;
    const int op = script[at];
    if (op == 0) {
      if (at + 6 > n_ints) return WEKWS_HIP_EINVAL;
      const int wire_call = script[at + 1], B = script[at + 2], width = script[at + 3], flush = script[at + 4], mcap = script[at + 5];
      if (B < 0 || B > max_streams || at + 6 + 2 * B > n_ints) return WEKWS_HIP_EINVAL;
      const int32_t* ids = script + at + 6;
      const int32_t* nsamp = ids + B;
      at += 6 + 2 * B;
      res[0] = wekws::resample_streams_plan(&S, bp, wire_call, 0, width, ids, nsamp, B, flush, mcap, &bad);
      res[1] = bad; res[2] = S.rows; res[3] = S.need_cap;
      if (res[0] == wekws::kResampleStreamsOk) {
        wekws::ResampleRow* const table = reinterpret_cast<wekws::ResampleRow*>(rows + int64_t(k) * max_streams * 12);
        const int32_t* pos = wekws::resample_slot_positions(&S, S.members_of.data(), B, num);
        wekws::resample_streams_push_rows(S, bp, wire_call, ids, nsamp, B, pos, table);
        wekws::resample_streams_commit(&S, ids, nsamp, B, flush, yields.data());
      }
    } else if (op == 1 || op == 2) {
      const int head = op == 2 ? 3 : 2;
      if (at + head > n_ints) return WEKWS_HIP_EINVAL;
      const int member = op == 2 ? script[at + 1] : -1, n = script[at + head - 1];
      if (n < 0 || at + head + n > n_ints || (op == 2 && (member < 0 || member >= num))) return WEKWS_HIP_EINVAL;
      res[1] = wekws::resample_streams_reset(&S, script + at + head, n, member);
      res[0] = res[1] >= 0;
      at += head + n;
    } else {
      return WEKWS_HIP_EINVAL;
    }
    for (int id = 0; id < max_streams; ++id) wekws::resample_streams_counts(S, id, counts + (int64_t(k) * max_streams + id) * 4);
  }
  return k;
}

// --------------------------------------------- resample bank ---------------------------------------------
// The plan of a rate bank, WITHOUT a device (resample_bank_plan.h alone).  dims[4]: LDS bytes of a launch, history capacity of a stream,
// max_out(nmax, flush), members.  With member_of_row (B) also the tile order of a launch over B rows of tiles_per_row tiles by `grid`
// workgroups: list_row / list_tile (B tiles_per_row) the (row, tile) of every list entry, span_begin (grid + 1) the first entry of every
// workgroup and the end of the list.  Returns 0, WEKWS_HIP_EINVAL for a bank no resampler has or a member index outside it,
// WEKWS_HIP_EUNSUPPORTED for a member that does not fit (*bad_member says which).
extern "C" int wekws_hip_debug_resample_bank_plan(const int32_t* rates, int num, int neu, int lpw, double rolloff, int nmax, int flush,
                                                  int64_t* dims, int* bad_member, const int32_t* member_of_row, int B, int tiles_per_row,
                                                  int grid, int32_t* list_row, int32_t* list_tile, int64_t* span_begin) {
  if (!dims || nmax < 0) return WEKWS_HIP_EINVAL;
  wekws::ResampleBankPlan bp;
  int bad = -1;
  const wekws::ResampleBankRefusal r = wekws::resample_bank_plan(rates, num, neu, lpw, rolloff, &bp, &bad);
  if (bad_member) *bad_member = bad;
  if (r == wekws::kResampleBankLds) return WEKWS_HIP_EUNSUPPORTED;
  if (r != wekws::kResampleBankOk) return WEKWS_HIP_EINVAL;
  dims[0] = wekws::resample_bank_lds_bytes(bp); dims[1] = wekws::resample_bank_hist_cap(bp);
  dims[2] = wekws::resample_bank_max_out(bp, nmax, flush); dims[3] = int64_t(bp.members.size());
  if (!member_of_row) return WEKWS_HIP_OK;
  if (B < 0 || tiles_per_row < 1 || grid < 1 || !list_row || !list_tile || !span_begin) return WEKWS_HIP_EINVAL;
  for (int b = 0; b < B; ++b)
    if (member_of_row[b] < 0 || member_of_row[b] >= num) return WEKWS_HIP_EINVAL;
  std::vector<int32_t> order(size_t(B) + 1);
  wekws::resample_bank_order(member_of_row, B, num, order.data());
  const int64_t total = wekws::resample_bank_total(B, tiles_per_row);
  for (int64_t t = 0; t < total; ++t) {
    list_row[t] = order[size_t(wekws::resample_bank_slot(t, tiles_per_row))];
    list_tile[t] = wekws::resample_bank_tile(t, tiles_per_row);
  }
  for (int w = 0; w <= grid; ++w) span_begin[w] = wekws::resample_bank_span_begin(total, grid, w);
  return WEKWS_HIP_OK;
}
// The rows of a rate-bank call, WITHOUT a device: the bank of (rates, encs) pairs (encs NULL: every member s16), then the function
// every compute and push call checks its rows with (resample_bank_plan.h: resample_bank_check_rows).  wire_call: a _wire call, width
// its row_bytes and pcm_addr the address of its bytes; otherwise an int16 / float call, width its nmax.  members (B): the member of
// every row (a push looks it up per stream); nsamp (B) or NULL; limit: the most samples of a row (a push: max_chunk).
// out[4]: the refusal (0: none; 1 pcm alignment, 2 row_bytes, 3 member, 4 length, 5 a row that is not s16 in an int16 / float call),
// the row it is about (-1: the call), bytes per sample of member 0, members.  Returns 0, or what the bank's own plan refuses with
// (WEKWS_HIP_EINVAL, WEKWS_HIP_EUNSUPPORTED; out[1] is then the member).
extern "C" int wekws_hip_debug_resample_bank_check_rows(const int32_t* rates, const int32_t* encs, int num, int neu, int lpw, double rolloff,
                                                        int wire_call, uint64_t pcm_addr, int64_t width, const int32_t* nsamp,
                                                        const int32_t* members, int B, int64_t limit, int64_t* out) {
  if (!out || B < 0 || (B > 0 && !members)) return WEKWS_HIP_EINVAL;
  wekws::ResampleBankPlan bp;
  int bad = -1;
  const wekws::ResampleBankRefusal r = wekws::resample_bank_plan(rates, encs, num, neu, lpw, rolloff, &bp, &bad);
  out[0] = 0; out[1] = bad; out[2] = 0; out[3] = 0;
  if (r == wekws::kResampleBankLds) return WEKWS_HIP_EUNSUPPORTED;
  if (r != wekws::kResampleBankOk) return WEKWS_HIP_EINVAL;
  out[0] = wekws::resample_bank_check_rows(bp, wire_call, pcm_addr, width, nsamp, members, B, limit, &bad);
  out[1] = bad; out[2] = bp.wire_bytes[0]; out[3] = int64_t(bp.members.size());
  return WEKWS_HIP_OK;
}
// Cap the grid of the handle's launches (max_grid <= 0: the handle's own again), so that a small batch makes one workgroup walk tiles of
// several members.
extern "C" int wekws_hip_debug_resample_bank_set_grid(wekws_hip_resample* r, int max_grid) {
  if (!r) return fail(WEKWS_HIP_EINVAL, "NULL handle");
  std::lock_guard<std::mutex> lk(r->mu);
  r->max_grid = max_grid > 0 ? max_grid : r->default_grid;
  return WEKWS_HIP_OK;
}

// --------------------------------------------- CTC keyword sets ---------------------------------------------
// A script of set operations on the table of ctc_kws_sets.h, WITHOUT a device: the table wekws_hip_ctc_kws_add_set / _drop_set /
// _assign decide every refusal and every id with.  vocab, n_streams: the handle's.  ops: n_ints int32, one operation after the other:
//   0, n_kw, n_tok, offsets[n_kw + 1], tokens[n_tok], ts_len (-1 - L: a NULL token set with token_set_len = L, so -1: none),
//      token_set[max(ts_len, 0)], threshold (two halves of the double, low first)
//                                                                  add: outcome = the set's id (the first add makes set 0), or -1
//   1, set                                                         drop: outcome 0, or -1
//   2, n, ids[n], sets[n]                                          assign: outcome 0, or -1
// outcomes: one per operation, at most max_ops.  image: the table afterwards (CtcSetTable::image), *image_len its length in ints; it is
// written only if it fits image_cap.  Returns the number of operations run, or WEKWS_HIP_EINVAL for a script that does not parse.
extern "C" int wekws_hip_debug_ctc_kws_sets(int vocab, int n_streams, const int32_t* ops, int64_t n_ints, int32_t* outcomes, int max_ops,
                                            int32_t* image, int64_t image_cap, int64_t* image_len) {
  if (vocab < 1 || n_streams < 0 || n_ints < 0 || (n_ints > 0 && !ops) || max_ops < 0 || (max_ops > 0 && !outcomes) || !image_len)
    return WEKWS_HIP_EINVAL;
  wekws::CtcSetTable tab;
  tab.init(vocab, n_streams);
  char why[256];
  int n = 0;
  int64_t i = 0;
  auto room = [&](int64_t k) { return k >= 0 && k <= n_ints - i; };
  while (i < n_ints) {
    if (n >= max_ops) return WEKWS_HIP_EINVAL;
    const int kind = ops[i++];
    if (kind == 0) {
      if (!room(2)) return WEKWS_HIP_EINVAL;
      const int n_kw = ops[i], n_tok = ops[i + 1];
      i += 2;
      if (n_kw < 0 || n_tok < 0 || !room(int64_t(n_kw) + 1 + n_tok + 1)) return WEKWS_HIP_EINVAL;
      const int32_t* offs = ops + i;
      const int32_t* toks = offs + n_kw + 1;
      // the table reads tokens up to the last offset: a script whose offsets run past its tokens is refused here, not there
      for (int k = 0; k <= n_kw; ++k)
        if (offs[k] > n_tok) return WEKWS_HIP_EINVAL;
      i += int64_t(n_kw) + 1 + n_tok;
      const int ts_len = ops[i++];
      if (!room(int64_t(ts_len < 0 ? 0 : ts_len) + 2)) return WEKWS_HIP_EINVAL;
      static const int32_t none = 0;
      const int32_t* ts = ts_len < 0 ? nullptr : (ts_len > 0 ? ops + i : &none);
      i += ts_len < 0 ? 0 : ts_len;
      double thr;
      std::memcpy(&thr, ops + i, 8);
      i += 2;
      outcomes[n++] = tab.add(wekws::CtcSetSpec{toks, offs, n_kw, ts, ts_len < 0 ? -1 - ts_len : ts_len, thr}, why, sizeof why);
    } else if (kind == 1) {
      if (!room(1)) return WEKWS_HIP_EINVAL;
      outcomes[n++] = tab.drop(ops[i++], why, sizeof why);
    } else if (kind == 2) {
      if (!room(1)) return WEKWS_HIP_EINVAL;
      const int cnt = ops[i++];
      if (cnt < 0 || !room(2 * int64_t(cnt))) return WEKWS_HIP_EINVAL;
      outcomes[n++] = tab.assign(ops + i, ops + i + cnt, cnt, why, sizeof why);
      i += 2 * int64_t(cnt);
    } else {
      return WEKWS_HIP_EINVAL;
    }
  }
  const std::vector<int32_t> img = tab.image();
  *image_len = int64_t(img.size());
  if (image && image_cap >= int64_t(img.size()) && !img.empty()) std::memcpy(image, img.data(), img.size() * 4);
  return n;
}
#endif  // WEKWS_TEST_HOOKS
