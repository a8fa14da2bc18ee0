// WHICH KERNEL RUNS A CALL -- pure functions, and the only place the choice is made.
//   * conv_schedule()  the blocks of a conv model: dilation, padding, cache slice and end-of-stack of each, cache length, longest
//     padding -- the one statement of it, usable from device code (ROUTE_HD); conv_workspace(): the scratch layout of a conv call;
//   * conv_route_flags()  what a conv model can run on, from its (built-shape) descriptor alone -- wekws_hip_create stores it;
//   * route_defaults() / apply_route_option()  the options of every backbone (wekws_hip_create, wekws_hip_set_option);
//   * select_conv_route() (flags, options, call) -> Route {family, tile count, split, context variant, fast, grid, threads, LDS
//     bytes, utterances per workgroup, head slices}, with the invariants of the choice checked (built widths, LDS within the CU's
//     160 KiB, the hand-over covering the longest padding, alignment preconditions);
//   * gru_shape_plan() / select_gru_route(): the GRU's built shape, and per call the family (exact f32, layer-major fp16, layer
//     wavefront), its launch geometry, where the non-finite pass runs and the scratch bytes; gru_reserve_bytes() for a reservation;
//   * fsmn_shape_plan() / select_fsmn_route(): the FSMN kernel's tile and, per tile, its frame tiles, utterances per workgroup, head
//     slices, grid and LDS bytes;
//   * effective_precision(): what wekws_hip_effective_precision reports, from the routes a model can take;
//   * plan_streams(): the plan of a wekws_hip_forward_streams call -- one table-driven launch (which kernel instance, which rows
//     share a workgroup) or the grouped path (which rows share a bucket).
// wekws_hip_forward (forward_conv / forward_gru / forward_fsmn) hands a route to its family's launcher, which executes it: the kernel variant, grid, threads and LDS from the
// route.  A launcher tests no eligibility of its own; it only refuses (-4, an internal error) a route whose threads or LDS bytes are
// not its kernel's or that names a variant it does not build.  So the geometry below restates every kernel header's (or the kernel
// headers take their constants from here), and the route the hooks trace records is the launch that ran.
// Plain C++ (no HIP): tests/test_route.py sweeps it on the CPU via the hooks library (wekws_hip_debug_conv_route,
// wekws_hip_debug_gru_route, wekws_hip_debug_fsmn_route); tests/test_hip_route_matrix.py checks the traced routes on the device.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/wekws_hip.h"

namespace wekws {

enum RouteFamily : int {
  ROUTE_NONE = 0,
  ROUTE_DS256_STREAM,      // ds256_stream.hip.h   chunks <= 16 frames, the stream's cache in LDS
  ROUTE_DS256_G32,         // ds256_g32.hip.h      exact f32, tile in registers, persistent
  ROUTE_DS256_MM,          // ds256_mm.hip.h       CTC-sized heads: classifier on the matrix cores
  ROUTE_DS256_G16,         // ds256_g16.hip.h      tile in registers (16 waves); ctx: with an incoming cache
  ROUTE_DS256_W16,         // ds256_w16.hip.h      LDS tile, 16 waves
  ROUTE_DS64_G4,           // ds64_g4.hip.h        one utterance per 4-wave workgroup; ctx
  ROUTE_MDTC64_STREAM,     // mdtc64_stream.hip.h  chunks <= 16 frames, two streams per workgroup
  ROUTE_MDTC64_G4,         // mdtc64_g4.hip.h <64> one utterance per 4-wave workgroup; ctx
  ROUTE_MDTC64_W16,        // mdtc64_w16.hip.h     LDS tile, 16 waves
  ROUTE_MDTC32_G4,         // mdtc64_g4.hip.h <32> one utterance per 2-wave workgroup; ctx
  ROUTE_DENSE_F16,         // dense_stack_f16.hip.h plain TCN on the matrix cores
  ROUTE_CONV_F16,          // conv_stack_f16.hip.h  LDS tile, 8 waves, any built width, split fp16
  ROUTE_CONV_F32,          // conv_stack.hip.h      LDS tile, 8 waves, any built width, exact f32
  ROUTE_FAMILIES
};

inline const char* route_family_name(int f) {
  static const char* const n[] = {"none", "ds256_stream", "ds256_g32", "ds256_mm", "ds256_g16", "ds256_w16", "ds64_g4", "mdtc64_stream",
                                  "mdtc64_g4", "mdtc64_w16", "mdtc32_g4", "dense_stack_f16", "conv_stack_f16", "conv_stack"};
  return f >= 0 && f < ROUTE_FAMILIES ? n[f] : "?";
}

// What the model's SHAPE admits (computed once, wekws_hip_create) ...
struct RouteFlags {
  int32_t cache_len, max_pad, kpre16;
  int32_t dils_1248;              // every block's dilation is 1, 2, 4 or 8 and its padding (kernel_size - 1) x dilation
  int32_t ds_stream_eligible;     // DS-TCN, C = 256, kernel size 8, dils_1248
  int32_t mdtc16_eligible;        // MDTC, C = 64, kernel size 5
  int32_t mdtc_stream_eligible;   // ... dils_1248, features <= 128 dims, both streams' caches fit the LDS
  int32_t mm_eligible;            // DS-TCN h256 with a per-frame linear head and paddings <= 56
  int32_t dense_ok;               // plain TCN whose paddings fit the dense-stack kernel's halo
  int32_t ds_stream_lds, mdtc_stream_lds;   // LDS bytes of the two streaming-step kernels for this cache (their headers' formulas)
  int32_t out_of_envelope;        // (any backbone) DEFAULT / F16X3 request, but the weights are outside the split-fp16 envelope
};
// ... what the options say (route_defaults; wekws_hip_set_option -> apply_route_option) ...
struct RouteOptions {
  int32_t w16_ok = 1;             // DS-TCN h256: the 16-wave kernels (WEKWS_HIP_OPT_W16 = 0: the generic 8-wave one)
  int32_t g16_ok = 1, g16_ctx = 1, g16_one_pass = 0;   // the register-resident kernels; their context variants; one pass (A/B aid)
  int32_t stream_ok = 1;          // chunks of <= 16 frames: the kernels with the LDS-resident cache
  int32_t mdtc16_ok = 1;          // MDTC h64: the 16-wave kernels
  int32_t mm_ok = 0;              // DS-TCN h256: the all-matrix-core kernel (ds256_mm)
  int32_t f32 = 0;                // precision F32, or the weights outside the split-fp16 envelope (and `envelope` on)
  int32_t split = 1;              // F16X3: three products; F16: one
  int32_t envelope = 1;           // WEKWS_HIP_OPT_ENVELOPE
  int32_t gru_pipe = 1;           // GRU: 1 the layer wavefront where it wins (select_gru_route), 2 wherever it fits, 0 never
  int32_t gru_nf_in_kernel = 1;   // GRU wavefront: its own non-finite workgroups where they fit (0: always the separate launch)
  int32_t head_slices = -1;       // FSMN / ds256_mm: head slices per tile of a small call: -1 automatic, 0 / 1 off, n forces n
};
// ... and the call (one tile of it)
struct RouteCall {
  int32_t B, T, ntiles;           // T: frames of THIS tile (<= WEKWS_HIP_TILE_FRAMES)
  int32_t has_in, has_out;        // caches
  int32_t x16;                    // features: 16-byte aligned rows in whole 4-float units (x % 16 == 0, row stride % 4 == 0)
  int32_t cache16;                // both cache pointers 16-byte aligned
  int32_t cus;
};
struct Route {
  int32_t family, nt, split, ctx, fast, grid, threads, lds_bytes, utts_per_wg;
  int32_t head_slices;            // ds256_mm: workgroups per utterance that share a CTC-sized head (0: off)
  const char* why_not;            // set when family == ROUTE_NONE: the invariant that failed
};

// ---- THE SCHEDULE of a conv model: which blocks, their dilations, paddings and cache slices, where a stack ends.  The kernels' block
// tables, the cache maps of a padded model, the any-shape path (generic.hip.h) and the non-finite path (nonfinite.hip.h, on the device:
// hence ROUTE_HD) all read it from here.
#ifdef __HIPCC__
#define ROUTE_HD __host__ __device__
#else
#define ROUTE_HD
#endif
ROUTE_HD inline int route_blocks(const wekws_hip_desc& d) {
  return d.backbone == WEKWS_HIP_BACKBONE_MDTC ? 1 + d.num_stack * d.stack_size : d.num_layers;
}
ROUTE_HD inline int route_dilation(const wekws_hip_desc& d, int i) {
  if (d.backbone == WEKWS_HIP_BACKBONE_MDTC) return i == 0 ? 1 : 1 << ((i - 1) % d.stack_size);   // mdtc.py:151-156, :229-237
  return 1 << i;                                                                                   // tcn.py:131-137
}
// block i closes a stack of an MDTC: its output joins the sum the classifier sees (mdtc.py:270-273)
ROUTE_HD inline bool route_stack_end(const wekws_hip_desc& d, int i) {
  return d.backbone == WEKWS_HIP_BACKBONE_MDTC && i > 0 && (i - 1) % d.stack_size == d.stack_size - 1;
}
// the dilations of blocks 0 .. i - 1, summed: a stack of S blocks holds 2^S - 1, block 0 of an MDTC stands before the stacks
ROUTE_HD inline int64_t route_dilations_before(const wekws_hip_desc& d, int i) {
  if (d.backbone != WEKWS_HIP_BACKBONE_MDTC) return (int64_t(1) << i) - 1;
  if (i == 0) return 0;
  const int S = d.stack_size;
  return 1 + int64_t((i - 1) / S) * ((int64_t(1) << S) - 1) + (int64_t(1) << ((i - 1) % S)) - 1;
}
struct ConvBlock {
  int32_t dil, pad, cache_off;    // padding (kernel_size - 1) x dilation = frames of its cache slice, which starts at cache_off
  int32_t zadd;                   // route_stack_end
};
struct ConvSchedule {
  wekws_hip_desc d;
  int32_t nb, max_pad;
  int64_t cache_len;              // (64 bits: create_generic checks a corrupt descriptor's against the int the kernels index with)
  ROUTE_HD ConvBlock block(int i) const {
    const int dil = route_dilation(d, i);
    return ConvBlock{dil, (d.kernel_size - 1) * dil, int32_t((d.kernel_size - 1) * route_dilations_before(d, i)), route_stack_end(d, i)};
  }
};
// (shifts by the depth of a stack: create_generic refuses depths beyond 24 before it asks)
ROUTE_HD inline ConvSchedule conv_schedule(const wekws_hip_desc& d) {
  ConvSchedule s{d, route_blocks(d), 0, (d.kernel_size - 1) * route_dilations_before(d, route_blocks(d))};
  for (int i = 0; i < s.nb; ++i) {
    const int64_t pad = int64_t(d.kernel_size - 1) * route_dilation(d, i);
    s.max_pad = pad > s.max_pad ? int32_t(pad < INT32_MAX ? pad : INT32_MAX) : s.max_pad;
  }
  return s;
}
inline int route_round_up(int v, int m) { return (v + m - 1) / m * m; }

inline RouteFlags conv_route_flags(const wekws_hip_desc& d, int ds_stream_lds, int mdtc_stream_lds) {
  RouteFlags f{};
  f.ds_stream_lds = ds_stream_lds;
  f.mdtc_stream_lds = mdtc_stream_lds;
  const int C = d.hdim, ks = d.kernel_size;
  const ConvSchedule s = conv_schedule(d);
  f.kpre16 = route_round_up(d.idim, 32);
  f.cache_len = int32_t(s.cache_len);
  f.max_pad = s.max_pad;
  f.dils_1248 = 1;
  for (int i = 0; i < s.nb; ++i)
    if (const int dil = route_dilation(d, i); !(dil == 1 || dil == 2 || dil == 4 || dil == 8)) f.dils_1248 = 0;
  f.dense_ok = d.backbone == WEKWS_HIP_BACKBONE_TCN && f.max_pad <= 56 && C <= 128;
  f.mdtc16_eligible = d.backbone == WEKWS_HIP_BACKBONE_MDTC && C == 64 && ks == 5;
  f.ds_stream_eligible = d.backbone == WEKWS_HIP_BACKBONE_DS_TCN && C == 256 && ks == 8 && f.dils_1248;
  f.mdtc_stream_eligible = f.mdtc16_eligible && f.kpre16 <= 128 && (64 * f.cache_len) % 4 == 0 && mdtc_stream_lds <= 158 * 1024 &&
                           f.dils_1248;
  f.mm_eligible = d.backbone == WEKWS_HIP_BACKBONE_DS_TCN && C == 256 && ks == 8 && f.max_pad <= 56 && d.head == WEKWS_HIP_HEAD_LINEAR;
  return f;
}

// ---- THE SCRATCH of a conv call, as byte offsets into the stream's workspace: the ping-pong caches that hand the causal context from
// one tile of a long input to the next, the global head's running sums (gsum; only where pooled), and -- a zero-padded model -- the
// widened copies of the caller's in / out caches.  d: the built shape; cache_len: its schedule's.  wekws_hip_workspace_bytes reports
// `bytes`, the forward takes its pointers from the offsets.
struct ConvWorkspace {
  int32_t ntiles, pooled;
  size_t cache[2], gsum, wide_in, wide_out, bytes;
};
inline ConvWorkspace conv_workspace(const wekws_hip_desc& d, int cache_len, int B, int T, bool padded) {
  ConvWorkspace w{};
  w.ntiles = (T + WEKWS_HIP_TILE_FRAMES - 1) / WEKWS_HIP_TILE_FRAMES;
  w.pooled = d.head == WEKWS_HIP_HEAD_GLOBAL;
  const size_t ce = size_t(B) * d.hdim * cache_len;
  const size_t wide = padded ? 2 * ce : 0;                  // the caller's caches, widened to the built channel count, in + out
  const size_t ge = w.pooled ? size_t(B) * d.hdim : 0;
  const size_t tiled = T <= WEKWS_HIP_TILE_FRAMES ? 0 : 2 * ce + ge;
  w.cache[1] = ce * sizeof(float);
  w.gsum = 2 * ce * sizeof(float);
  w.wide_in = tiled * sizeof(float);
  w.wide_out = (tiled + ce) * sizeof(float);
  w.bytes = (tiled + wide) * sizeof(float);
  return w;
}

// The product's options for a model (any backbone; f: conv_route_flags, or zero but for out_of_envelope)
inline RouteOptions route_defaults(const wekws_hip_desc& d, const RouteFlags& f) {
  RouteOptions o;
  o.mdtc16_ok = f.mdtc16_eligible;
  // ds256_mm: on for CTC-sized heads (its activation planes feed an MFMA classifier directly), off for keyword heads (the 16-wave
  // kernel is 12 % faster there)
  o.mm_ok = f.mm_eligible && d.odim > 16;
  o.f32 = d.precision == WEKWS_HIP_PRECISION_F32 || f.out_of_envelope;
  o.split = d.precision != WEKWS_HIP_PRECISION_F16;
  return o;
}
// One WEKWS_HIP_OPT_* (include/wekws_hip.h) -> 0, or -1 for an option that does not exist
inline int apply_route_option(RouteOptions& o, const wekws_hip_desc& d, const RouteFlags& f, int option, int value) {
  switch (option) {
    case WEKWS_HIP_OPT_W16: o.w16_ok = value != 0; break;
    case WEKWS_HIP_OPT_MDTC16: o.mdtc16_ok = f.mdtc16_eligible && value != 0; break;
    case WEKWS_HIP_OPT_STREAM: o.stream_ok = value != 0; break;
    case WEKWS_HIP_OPT_MM: o.mm_ok = f.mm_eligible && (value < 0 ? d.odim > 16 : value != 0); break;
    case WEKWS_HIP_OPT_HEAD_SLICES: o.head_slices = value; break;
    // (2: one workgroup per utterance; 3: no context variants -- measurement aids)
    case WEKWS_HIP_OPT_G16: o.g16_ok = value != 0; o.g16_one_pass = value == 2; o.g16_ctx = value != 3; break;
    case WEKWS_HIP_OPT_ENVELOPE:
      o.envelope = value != 0;
      o.f32 = d.precision == WEKWS_HIP_PRECISION_F32 || (f.out_of_envelope && o.envelope);
      break;
    case WEKWS_HIP_OPT_GRU_PIPE: o.gru_pipe = value < 0 ? 1 : value > 2 ? 2 : value; break;
    default: return -1;
  }
  return 0;
}

// The shape a conv model RUNS as (wekws_hip_create): as it is, zero-padded to the next built width / kernel size (exact: see
// pad_conv_shape in weight_image.hip.h), or on the any-shape path of generic.hip.h.
enum : int { SHAPE_AS_IS = 0, SHAPE_PADDED = 1, SHAPE_GENERIC = 2 };
struct ShapePlan {
  int32_t kind, C, ks;            // SHAPE_PADDED: the built width / kernel size it runs as
  const char* why;                // SHAPE_GENERIC: the limit it exceeds
};
inline ShapePlan conv_shape_plan(const wekws_hip_desc& d, int max_blocks) {
  ShapePlan p{SHAPE_AS_IS, d.hdim, d.kernel_size, nullptr};
  const int C = d.hdim, ks = d.kernel_size;
  const bool mdtc = d.backbone == WEKWS_HIP_BACKBONE_MDTC;
  const int ks_built = mdtc ? 5 : 8;                          // the kernel sizes of the reference recipes ({ds_tcn,tcn}.yaml: 8; mdtc*.yaml: 5)
  auto generic = [&](const char* why) { p.kind = SHAPE_GENERIC; p.why = why; return p; };
  // built widths: 64 / 128 / 256, and 32 for MDTC (mdtc_small.yaml; DS-TCN / TCN with 32 channels run as 64: round-5 defect 2)
  const bool odd_c = C != 64 && C != 128 && C != 256 && !(C == 32 && mdtc);
  if (odd_c || (ks >= 1 && ks < ks_built)) {
    if (C > 256) return generic("wider than any built kernel (256 channels)");
    if (ks > ks_built) return generic("kernel size above the built one");
    const int Cp = !odd_c ? C : (C < 32 && mdtc) ? 32 : C < 64 ? 64 : C < 128 ? 128 : 256;
    if (mdtc && Cp > 128) return generic("MDTC wider than 128 channels does not fit the LDS tile");
    if (route_blocks(d) > max_blocks) return generic("more residual blocks than the cache maps hold");
    if (odd_c && d.head == WEKWS_HIP_HEAD_IDENTITY) return generic("identity head on a padded width (y is the tile itself)");
    p.kind = SHAPE_PADDED; p.C = Cp; p.ks = ks_built;
    return p;
  }
  if (mdtc && C == 256) return generic("MDTC with 256 channels does not fit the LDS tile");
  if (ks != ks_built) return generic("kernel size above the built one");
  if (d.precision != WEKWS_HIP_PRECISION_F32 && route_blocks(d) > max_blocks) return generic("more residual blocks than the split-fp16 kernels track maxima for");
  return p;
}

// frame tiles of 16 columns a call of T frames takes: 1, 2, 4 or 7
inline int route_nt(int T) {
  const int nt16 = (T + 15) / 16;
  return nt16 <= 1 ? 1 : nt16 <= 2 ? 2 : nt16 <= 4 ? 4 : 7;
}

// d: the descriptor of the shape the kernels RUN (after zero-padding to a built width / kernel size).
inline Route select_conv_route(const wekws_hip_desc& d, const RouteFlags& f, const RouteOptions& o, const RouteCall& c) {
  Route r{};
  const int ds_stream_lds = f.ds_stream_lds, mdtc_stream_lds = f.mdtc_stream_lds;
  const int C = d.hdim, ks = d.kernel_size, K = d.odim;
  const int nt = route_nt(c.T);
  const bool f16 = !o.f32;
  const bool has_in = c.has_in != 0;
  const bool linear2 = d.head == WEKWS_HIP_HEAD_LINEAR && K <= 2;
  const bool x_items = d.idim % 8 == 0 && c.x16;                 // whole aligned 8-float feature items
  const bool pooled = d.head == WEKWS_HIP_HEAD_GLOBAL || d.head == WEKWS_HIP_HEAD_LAST;
  auto fail = [&](const char* why) { r = Route{}; r.why_not = why; return r; };
  auto done = [&](int family, int nt_, bool ctx, bool fast, int grid, int threads, int lds, int upw) {
    // split 0 (one fp16 product) only where the family HAS that variant: ds256_mm, dense_stack_f16 and conv_stack_f16 run their
    // three products whatever the precision asks (tests/test_hip_route_matrix.py's F16 control tells the two apart on the device)
    const bool one_product = family == ROUTE_DS256_STREAM || family == ROUTE_DS256_G16 || family == ROUTE_DS256_W16 || family == ROUTE_DS64_G4 ||
                             family == ROUTE_MDTC64_STREAM || family == ROUTE_MDTC64_G4 || family == ROUTE_MDTC64_W16 || family == ROUTE_MDTC32_G4;
    r.family = family; r.nt = nt_; r.split = o.split || !one_product; r.ctx = ctx; r.fast = fast; r.grid = grid; r.threads = threads; r.lds_bytes = lds;
    r.utts_per_wg = upw;
    return r;
  };
  if (c.B <= 0 || c.T <= 0 || c.T > WEKWS_HIP_TILE_FRAMES) return fail("tile of 1 .. 112 frames");
  if (!(C == 32 || C == 64 || C == 128 || C == 256)) return fail("hidden width is not a built one (32 / 64 / 128 / 256): wekws_hip_create pads");
  const int ks_built = d.backbone == WEKWS_HIP_BACKBONE_MDTC ? 5 : 8;
  if (ks != ks_built) return fail("kernel size is not the built one: wekws_hip_create pads or takes the any-shape path");

  // LDS bytes of every family, its header's geometry restated (a launcher refuses a route whose LDS is not its kernel's)
  const int tt = 16 * nt, SS = (nt % 2) ? tt : tt + 16;             // frames of the tile; Geom<>'s row stride
  const int U = C >= 128 ? 1 : 128 / C, KC = C >= 64 ? 32 : 16;
  const int R = d.backbone == WEKWS_HIP_BACKBONE_MDTC ? (C > 2 * KC ? C : 2 * KC) : 2 * KC;
  const int tile_lds = (U * C * SS + U * R * SS) * 4;                // Geom<>: conv_stack and conv_stack_f16
  auto w16_lds = [](int ntk) { return 1280 * 16 * ntk + 4096; };      // W16Geom<NT>: 4 operand planes of 64 TT bytes + 256 rows of TT + 4 floats
  const int mm_lds = 1280 * tt + 2 * 8 * 56 * 16;                    // MmGeom<NT>: the same planes and slab + 2 left-context planes
  const int m16_lds = (2 * 64 * SS * (nt <= 2 ? 2 : 1) + 2 * 64 * (tt + 4)) * 4;   // M16Geom<NT>: Geom<MDTC, 64>'s slab (twice for <= 2 tiles) + 2 x 64 rows
  const int dense_lds = U * (2 * (C / 8) * (56 + tt) * 16 + 2 * 4 * tt * 16);     // DenseGeom<>: hi / lo planes of h + 2 staged K steps of x
  const int nt_g4 = has_in && nt <= 4 ? 4 : nt;                     // *_g4: the context variant's tile is one 16-lane row, >= 4 tiles
  const int g4_lds = 2 * (C / 8) * 16 * nt_g4 * 16;                  // 2 Plane<C, 16 NT>

  switch (d.backbone) {
    case WEKWS_HIP_BACKBONE_DS_TCN: {
      const bool strm = f16 && f.ds_stream_eligible && o.w16_ok && !o.mm_ok && o.stream_ok && c.ntiles == 1 && c.T <= 16 &&
                        (c.has_in || c.has_out) && c.cache16 && ds_stream_lds <= 160 * 1024;
      if (strm) {
        if (256 * f.cache_len > 7 * 4 * 1024) return fail("ds256_stream: a stream's cache is more than seven 16-byte items per thread");
        return done(ROUTE_DS256_STREAM, 1, true, false, c.B, 1024, ds_stream_lds, 1);
      }
      const bool reg_ok = C == 256 && o.w16_ok && o.g16_ok && f.ds_stream_eligible;   // the register-resident kernels' model side
      const bool fast = linear2 && f.kpre16 <= 64 && x_items;
      if (!f16) {
        if (reg_ok && !has_in && fast) return done(ROUTE_DS256_G32, nt, false, true, c.B < c.cus || o.g16_one_pass ? c.B : c.cus, 1024, w16_lds(nt), 1);
        if (tile_lds > 160 * 1024) return fail("conv_stack: tile beyond the LDS");
        return done(ROUTE_CONV_F32, nt, has_in, false, (c.B + U - 1) / U, 512, tile_lds, U);
      }
      if (o.mm_ok) {
        if (!f.mm_eligible) return fail("ds256_mm on a model it is not built for");
        done(ROUTE_DS256_MM, nt, has_in, false, c.B, 1024, mm_lds, 1);
        // a CTC-sized head on a handful of streams: up to 8 workgroups per utterance share its o-tiles (ds256_mm.hip.h)
        if (d.odim >= 256 && c.B * 2 <= c.cus) r.head_slices = o.head_slices >= 0 ? o.head_slices : (c.cus / c.B > 8 ? 8 : c.cus / c.B);
        return r;
      }
      if (reg_ok && (!has_in || (o.g16_ctx && nt >= 2))) {
        const int ntk = has_in && nt < 4 ? 4 : nt;                   // the context tile is one 16-lane row: >= 4 tiles
        if (!has_in) return done(ROUTE_DS256_G16, ntk, false, fast, fast && !o.g16_one_pass && c.B > c.cus ? c.cus : c.B, 1024, w16_lds(ntk), 1);
        if (fast) return done(ROUTE_DS256_G16, ntk, true, true, !o.g16_one_pass && c.B > c.cus ? c.cus : c.B, 1024, w16_lds(ntk), 1);
        // (other heads / feature layouts with an incoming cache: the LDS-tile kernel below)
      }
      if (C == 256 && o.w16_ok) {
        // the hand-over of ds256_w16 walks a block's slice in passes of 64 columns: any padding is covered (round-5 defect 1)
        return done(ROUTE_DS256_W16, nt, has_in, false, c.B, 1024, w16_lds(nt), 1);
      }
      if (C == 64 && o.g16_ok && d.num_layers <= 4 && f.dils_1248 && (!has_in || (o.g16_ctx && nt >= 2)) && linear2 && f.kpre16 <= 96 && x_items) {
        if (has_in && !(nt <= 4 || nt == 7)) return fail("ds64_g4 context variant: 4 or 7 tiles");
        return done(ROUTE_DS64_G4, nt_g4, has_in, true, c.B, 256, g4_lds, 1);
      }
      return done(ROUTE_CONV_F16, nt, has_in, false, (c.B + U - 1) / U, 512, tile_lds, U);
    }
    case WEKWS_HIP_BACKBONE_TCN:
      if (!f16) return done(ROUTE_CONV_F32, nt, has_in, false, (c.B + U - 1) / U, 512, tile_lds, U);
      if (f.dense_ok) return done(ROUTE_DENSE_F16, nt, has_in, false, (c.B + U - 1) / U, 512, dense_lds, U);
      return done(ROUTE_CONV_F16, nt, has_in, false, (c.B + U - 1) / U, 512, tile_lds, U);
    case WEKWS_HIP_BACKBONE_MDTC: {
      const bool m16 = f16 && o.mdtc16_ok && f.mdtc16_eligible;
      if (m16 && f.mdtc_stream_eligible && o.stream_ok && c.ntiles == 1 && c.T <= 16 && (c.has_in || c.has_out) && c.cache16 && x_items)
        return done(ROUTE_MDTC64_STREAM, 1, true, false, (c.B + 1) / 2, 1024, mdtc_stream_lds, 2);
      const bool head_ok = linear2 || (pooled && d.head_hidden <= 448);
      if (m16 && o.g16_ok && f.mdtc_stream_eligible && (!has_in || (o.g16_ctx && nt >= 2 && (c.B > 2 || nt < 7))) && head_ok && f.kpre16 <= 96 &&
          x_items && (!has_in || linear2))
        return done(ROUTE_MDTC64_G4, nt_g4, has_in, true, c.B, 256, g4_lds, 1);
      if (m16) return done(ROUTE_MDTC64_W16, nt, has_in, false, (c.B + 1) / 2, 1024, m16_lds, 2);
      if (f16 && C == 32 && o.g16_ok && d.stack_size <= 4 && f.dils_1248 && (!has_in || (o.g16_ctx && nt >= 2)) && head_ok && f.kpre16 <= 64 && x_items &&
          (!has_in || linear2))
        return done(ROUTE_MDTC32_G4, nt_g4, has_in, true, c.B, 128, g4_lds, 1);
      if (f16) {
        if (C > 128) return fail("MDTC wider than 128 channels does not fit the LDS tile: any-shape path");
        return done(ROUTE_CONV_F16, nt, has_in, false, (c.B + U - 1) / U, 512, tile_lds, U);
      }
      if (tile_lds > 160 * 1024) return fail("conv_stack: tile beyond the LDS");
      return done(ROUTE_CONV_F32, nt, has_in, false, (c.B + U - 1) / U, 512, tile_lds, U);
    }
    default:
      return fail("not a conv backbone");
  }
}


// ---------------------------------------------------------------------------------------------------------------------------------
// GRU (gru.hip.h: exact f32; gru_f16.hip.h: layer-major split fp16; gru_pipe.hip.h: the layer wavefront).  The kernel headers take
// the constants below from here; the sizes of GruF16Geom<NN> are restated (gru_f16.hip.h asserts that they agree).
constexpr int kGruMaxLayers = 4;
constexpr int kGruH = 128;                                    // the built hidden size
constexpr int kGruPipeMaxSlots = 128;
constexpr int kGruPipeRingLog = 4, kGruPipeRing = 1 << kGruPipeRingLog;
constexpr int kGruPipeGiStep = 8 * 4 * 1024;                  // bytes of one step of gate granules: [wave][item][lane][16]
constexpr int kGruPipeHStep = 16 * 16 * 64;                   // bytes of one step of state granules: [k-octet][stream][8][8]
#ifndef WEKWS_GRU_MAX_PACKED_WGS
#define WEKWS_GRU_MAX_PACKED_WGS 128
#endif
constexpr int kGruMaxPackedWgs = WEKWS_GRU_MAX_PACKED_WGS;
constexpr int gru_f16_seq_step(int nn) { return 2 * (kGruH / 8) * 16 * nn * 16; }   // GruF16Geom<NN>::SEQ_STEP (bytes)
constexpr int gru_f16_gi_step(int nn) { return 8 * 3 * nn * 256; }                  // GruF16Geom<NN>::GI_STEP (floats)
constexpr int kGruF16Cs = 4;                                                         // GruF16Geom<NN>::CS
constexpr int gru_f16_lds_bytes(int nn) { return 2 * kGruF16Cs * gru_f16_seq_step(nn); }
inline int gru_f32_lds_bytes(int kpre, int nlayers, int nn) {                        // GruGeom<NN>::lds_bytes
  return (kpre + (1 + nlayers) * kGruH) * ((nn % 2) ? 16 * nn : 16 * nn + 16) * 4;
}

// The shape a GRU RUNS as (wekws_hip_create): as it is, zero-padded to the built hidden size (exact: see pad_gru_hidden in
// weight_image.hip.h), or on the any-shape path of generic.hip.h.  (ShapePlan::C: the built hidden size.)
inline ShapePlan gru_shape_plan(const wekws_hip_desc& d) {
  ShapePlan p{SHAPE_AS_IS, d.hdim, d.kernel_size, nullptr};
  auto generic = [&](const char* why) { p.kind = SHAPE_GENERIC; p.why = why; return p; };
  if (d.num_layers > kGruMaxLayers) return generic("more layers than the GRU kernels' tables (4)");
  if (d.head != WEKWS_HIP_HEAD_LINEAR) return generic("pooled / identity head on a GRU");
  if (d.hdim > kGruH) return generic("hidden size above the built 128");
  if (d.hdim < kGruH) { p.kind = SHAPE_PADDED; p.C = kGruH; }
  return p;
}

// split fp16 (layer-major kernels and the wavefront): features and classifier of <= 128 dims
inline bool gru_f16_ok(const wekws_hip_desc& d) { return route_round_up(d.idim, 32) <= 128 && d.odim <= 128; }

// Streams per workgroup of a streaming chunk (T <= 16, single launch).  A workgroup's time does not depend on how many of
// its 16 MFMA columns are real, but the time-parallel passes pack (step, stream) pairs into the columns when it owns <= 8
// streams (gru_f16_kernel: TIME-PACKED mode) -- so with CUs to spare, fewer streams per workgroup is less work per
// workgroup: 256 streams as 128 workgroups of 2 instead of 16 of 16.  Capped at kGruMaxPackedWgs workgroups: every one
// streams the layers' 1.6 MB of weights from L2.
inline int gru_f16_spw(int B, int T, int cus) {
  if (T > 16 || B <= 1) return 16;
  const int wgs = cus < kGruMaxPackedWgs ? cus : kGruMaxPackedWgs;
  int spw = 1;
  while (spw < 16 && spw * wgs < B) spw *= 2;
  return spw;
}
// stream tiles per workgroup of the layer-major kernels: one (16 streams) until every CU has a workgroup, then two
inline int gru_f16_nn(int B) { return B > 16 * 256 ? 2 : 1; }

// ---- the wavefront's geometry of one call: stream slots per workgroup, tiles, resident slots ----
struct GruPipeGeom {
  int stages, spw, tiles, slots, slots_p;
};
inline bool gru_pipe_geom(int nlayers, int B, int T, int cus, GruPipeGeom* g) {
  g->stages = 2 * nlayers;
  int smax = cus / g->stages;
  smax = smax > kGruPipeMaxSlots ? kGruPipeMaxSlots : smax;
  if (smax < 1 || nlayers > kGruMaxLayers) return false;
  // streaming chunks (T <= 16): fewer streams per tile while every tile still gets its own slot -- a workgroup's time does
  // not depend on how many of its 16 MFMA columns are real, and tiles of <= 8 streams run the first stage time-packed (all
  // steps in one or two MFMA tiles).  Longer inputs: full tiles -- a time-packed first stage makes ALL steps before the
  // recurrence sees the first one (measured at B = 256 x 98 frames: 0.67x of the layer-major kernels)
  int spw = T <= 16 ? 1 : 16;
  while (spw < 16 && (B + spw - 1) / spw > smax) spw *= 2;
  g->spw = spw;
  g->tiles = (B + spw - 1) / spw;
  g->slots = g->tiles < smax ? g->tiles : smax;
  g->slots_p = (g->slots + 7) / 8 * 8;                       // block b runs on XCD b % 8: a slot's stages share an XCD
  return true;
}
// bytes of one call: the plain workspace behind the control words (seq_in, seq_top, sc: each per slot) and the granule
// workspace (gi per layer, state granules per layer below the top: a ring per slot each)
struct GruPipeBytes {
  size_t seq, sc, gi, hs;
  size_t plain() const { return 2 * seq + sc; }
  size_t granules(int nlayers) const { return size_t(nlayers) * gi + size_t(nlayers - 1) * hs; }
};
inline size_t route_align256(size_t v) { return (v + 255) / 256 * 256; }
inline GruPipeBytes gru_pipe_bytes(const GruPipeGeom& g, int T) {
  GruPipeBytes b;
  b.seq = route_align256(size_t(g.slots) * T * gru_f16_seq_step(1));
  b.sc = route_align256(size_t(g.slots) * T * 16 * sizeof(float));
  b.gi = route_align256(size_t(g.slots) * kGruPipeRing * kGruPipeGiStep);
  b.hs = route_align256(size_t(g.slots) * kGruPipeRing * kGruPipeHStep);
  return b;
}

enum : int { GRU_NONE = 0, GRU_F32 = 1, GRU_F16 = 2, GRU_PIPE = 3 };
inline const char* gru_family_name(int f) {
  static const char* const n[] = {"none", "gru_f32", "gru_f16", "gru_pipe"};
  return f >= 0 && f <= GRU_PIPE ? n[f] : "?";
}
struct GruCall {
  int32_t B, T;
  int32_t x16;                    // features 16-byte aligned (the wavefront's two-K-step variant loads whole octets)
  int32_t padded;                 // the model runs zero-padded (gru_shape_plan): widened copies of the caller's states, in + out
  int32_t cus;
};
struct GruRoute {
  int32_t family;
  int32_t nn, spw;                // GRU_F32 / GRU_F16: stream tiles of 16 per workgroup; streams per workgroup
  int32_t chunked, tchunk, nchunks;   // GRU_F16: the time-parallel passes as launches over (tile x time chunk), or one launch
  int32_t stages, slots, slots_p, tiles, pk, k2;   // GRU_PIPE (tiles: every family's stream tiles)
  int32_t nf_in_kernel;           // the non-finite pass: inside the wavefront launch (its own workgroups), else its own launch
  int32_t grid, lds_bytes;        // (GRU_F16: of a single launch)
  size_t plain_bytes, granule_bytes;   // the call's scratch: the stream's workspace, and its granule buffer (GRU_PIPE)
  size_t seq_bytes, gi_bytes, hs_bytes;   // ... carved into: two layer sequences, gate pre-activations (GRU_PIPE: per layer),
                                          // state granules (GRU_PIPE: per layer below the top), 256-byte aligned
  const char* why_not;
};

// d: the descriptor of the shape the kernels RUN (hidden size 128).
inline GruRoute select_gru_route(const wekws_hip_desc& d, const RouteOptions& o, const GruCall& c) {
  GruRoute r{};
  const int L = d.num_layers, B = c.B, T = c.T;
  auto fail = [&](const char* why) { r = GruRoute{}; r.why_not = why; return r; };
  if (B <= 0 || T <= 0) return fail("no streams or no frames");
  if (d.hdim != kGruH || L < 1 || L > kGruMaxLayers) return fail("not the built GRU shape: wekws_hip_create pads or takes the any-shape path");
  const size_t padded = c.padded ? 2 * size_t(L) * B * kGruH * sizeof(float) : 0;
  if (o.f32 || !gru_f16_ok(d)) {
    // exact f32 (gru.hip.h): 64-stream tiles amortise the per-step weight stream 4x better but need B large enough to fill the chip
    const int kpre = route_round_up(d.idim, 16);
    if (kpre > 128) return fail("gru_f32: features of more than 128 dims");
    r.family = GRU_F32;
    r.nn = B >= 64 * 256 && gru_f32_lds_bytes(kpre, L, 4) <= 160 * 1024 ? 4 : 1;
    r.spw = 16 * r.nn;
    r.tiles = r.grid = (B + r.spw - 1) / r.spw;
    r.lds_bytes = gru_f32_lds_bytes(kpre, L, r.nn);
    if (r.lds_bytes > 160 * 1024) return fail("gru_f32: tile beyond the LDS");
    r.plain_bytes = padded;
    return r;
  }
  // the layer wavefront: where every tile of streams gets its own slot, or a few rounds of slots -- many more tiles than
  // resident slots and every workgroup serves several tiles one after the other (each round fills and drains the pipeline);
  // beyond ~8 rounds the layer-major kernels (all CUs on every pass, two tiles per workgroup) win -- measured with the ring
  // buffers, 2 layers: 1.65x at B = 2048 (2 rounds), 1.31x at 4096, 1.09x at 8192 (8 rounds), 0.96x at B = 16384 (16 rounds);
  // option value 2 runs the wavefront wherever it fits.  (A slot's steps of one launch are numbered in an int: T < 2^24.)
  GruPipeGeom g;
  if (o.gru_pipe && T < (1 << 24) && gru_pipe_geom(L, B, T, c.cus, &g) && (g.tiles <= 8 * g.slots || o.gru_pipe == 2)) {
    r.family = GRU_PIPE;
    r.stages = g.stages; r.spw = g.spw; r.tiles = g.tiles; r.slots = g.slots; r.slots_p = g.slots_p;
    // <2>: at most two K steps of features in whole, 16-byte aligned octets (the 40-d / 64-d front ends); <4>: anything else
    r.k2 = route_round_up(d.idim, 32) <= 64 && d.idim % 8 == 0 && c.x16;
    r.pk = g.spw <= 8;                                       // time-packed first stage
    // Non-finite pass: the wavefront's own extra workgroups (one per slot) where there are CUs left for them to run BESIDE the
    // pipeline -- streaming chunks, small batches: no second launch, 2.68 -> 2.48 us per frame at B = 1 --; where the stage
    // workgroups fill the device they would only start behind it and scan 16 streams each (measured at B = 1024 x 98:
    // 0.186 ms against 0.176 with the separate launch, whose 1024 small workgroups scan in parallel): the launch stays.
    // A slot's non-finite workgroup scans the streams of ONE tile: every tile must have a slot of its own.
    r.nf_in_kernel = o.gru_nf_in_kernel && (g.stages + 1) * g.slots <= c.cus && g.tiles <= g.slots;
    r.grid = g.stages * g.slots_p + (r.nf_in_kernel ? g.slots : 0);
    r.lds_bytes = 128 * 1024 + 1024;                         // kGruPipeLds (gru_pipe.hip.h)
    const GruPipeBytes pb = gru_pipe_bytes(g, T);
    r.plain_bytes = pb.plain() + padded;
    r.granule_bytes = pb.granules(L);
    r.seq_bytes = pb.seq; r.gi_bytes = pb.gi; r.hs_bytes = pb.hs;
    return r;
  }
  // the layer-major kernels (gru_f16.hip.h)
  r.family = GRU_F16;
  r.nn = gru_f16_nn(B);
  r.spw = r.nn == 2 ? 32 : gru_f16_spw(B, T, c.cus);
  r.tiles = (B + r.spw - 1) / r.spw;
  // few stream tiles and a long input: the time-parallel passes over (tile x time chunk) so that every CU works
  const int tiles16 = (B + 16 * r.nn - 1) / (16 * r.nn);
  r.chunked = 2 * tiles16 <= c.cus && T >= 32;
  r.tchunk = T; r.nchunks = 1;
  if (r.chunked) {
    int nchunks = (2 * c.cus + tiles16 - 1) / tiles16;
    int tchunk = ((T + nchunks - 1) / nchunks + kGruF16Cs - 1) / kGruF16Cs * kGruF16Cs;
    if (tchunk < 2 * kGruF16Cs) tchunk = 2 * kGruF16Cs;
    r.tchunk = tchunk;
    r.nchunks = (T + tchunk - 1) / tchunk;
  }
  r.grid = r.tiles;
  r.lds_bytes = gru_f16_lds_bytes(r.nn);
  const size_t seq = size_t(r.tiles) * T * gru_f16_seq_step(r.nn), gi = size_t(r.tiles) * T * gru_f16_gi_step(r.nn) * sizeof(float),
               sc = size_t(r.tiles) * T * 16 * sizeof(float);
  r.seq_bytes = route_align256(seq); r.gi_bytes = route_align256(gi);
  r.plain_bytes = 2 * r.seq_bytes + r.gi_bytes + route_align256(sc) + padded;
  return r;
}

// What a reservation for "calls of up to (B, T)" has to hold: a call's scratch is not monotonic -- a GRU chunk of <= 16 frames
// spreads its streams over more, smaller workgroups (gru_f16_spw), so (256, 10) needs more than (256, 20) and (128, 10) as much
// as (256, 10) -- so the maximum over the shapes where the geometry changes is taken: the frame counts {T, min(T, 16)} and the
// stream counts B, the packed-workgroup boundaries 2^k x (workgroups) below B, the two-tiles-per-workgroup threshold, and the
// wavefront's most slots (= most rings) with one stream per tile.  (tests/test_route.py sweeps every call below (B, T).)
inline void gru_reserve_bytes(const wekws_hip_desc& d, const RouteOptions& o, const GruCall& c, size_t* plain, size_t* gran) {
  *plain = *gran = 0;
  const int B = c.B, T = c.T;
  const int ts[2] = {T, T < 16 ? T : 16};
  int bs[12], nb = 0;
  bs[nb++] = B;
  const int wgs = c.cus < kGruMaxPackedWgs ? c.cus : kGruMaxPackedWgs;
  for (int k = 1; k <= 16; k *= 2)
    if (k * wgs < B) bs[nb++] = k * wgs;
  if (16 * 256 < B) bs[nb++] = 16 * 256;
  GruPipeGeom g;
  if (gru_pipe_geom(d.num_layers, 1 << 30, 1, c.cus, &g)) {
    if (g.slots < B) bs[nb++] = g.slots;
    if (16 * g.slots + 1 <= B) bs[nb++] = 16 * g.slots + 1;
  }
  for (int i = 0; i < nb; ++i)
    for (int j = 0; j < 2; ++j) {
      GruCall k = c;
      k.B = bs[i]; k.T = ts[j];
      const GruRoute r = select_gru_route(d, o, k);
      *plain = r.plain_bytes > *plain ? r.plain_bytes : *plain;
      *gran = r.granule_bytes > *gran ? r.granule_bytes : *gran;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// FSMN (fsmn_f16.hip.h, the block-floating split-fp16 kernel; the kernel header takes these constants from here)
constexpr int kFsmnMaxLayers = 16;
constexpr int kFsmnMaxTaps = 32;
constexpr int kFsmnTileFrames = 64;
constexpr int kFsmnLdsLimit = 160 * 1024 - 2048;   // (the maxima cells are static LDS beside the dynamic tile)

// channel counts padded to multiples of 32 (taps_ld: of 4) -- FsmnParams' padded sizes
struct FsmnDims {
  int32_t kin, a1p, linp, dp, a2p, op, taps_ld;
};
// FsmnLds::make(P, TT, U).bytes() restated: the LDS of a tile of TT frames = U utterances x TT / U frames
inline int fsmn_lds_bytes(const FsmnDims& q, int TT, int U) {
  const int seg = (TT / U + q.taps_ld + 3) / 4 * 4;
  const int ss = (U * seg + 7) / 8 * 8 + 4;
  const int xb = q.kin * TT * 4, linb = q.linp * TT * 4, mb = q.dp * TT * 4;
  const int r0 = xb > linb + mb ? xb : linb + mb;
  int r1 = q.a1p * TT * 4;
  if (q.dp * ss * 4 > r1) r1 = q.dp * ss * 4;
  if (q.a2p * TT * 4 > r1) r1 = q.a2p * TT * 4;
  return r0 + r1;
}
struct FsmnPlan {
  int32_t kind;                   // SHAPE_AS_IS or SHAPE_GENERIC
  int32_t max_nt;                 // most 16-frame tiles per utterance whose LDS fits: frames of one kernel call = 16 max_nt
  FsmnDims q;
  const char* why;                // SHAPE_GENERIC: the limit it exceeds
};
// The create_fsmn choices that need no weights (weights outside the split-fp16 envelope take the any-shape path as well)
inline FsmnPlan fsmn_shape_plan(const wekws_hip_desc& d) {
  FsmnPlan p{};
  const int ntaps = d.kernel_size + d.stack_size;
  p.q = FsmnDims{route_round_up(d.idim, 32), route_round_up(d.aux[0], 32), route_round_up(d.hdim, 32), route_round_up(d.num_stack, 32),
                 route_round_up(d.aux[1], 32), route_round_up(d.odim, 32), route_round_up(ntaps, 4)};
  auto generic = [&](const char* why) { p.kind = SHAPE_GENERIC; p.why = why; return p; };
  // precision F32 is served with the reference's own arithmetic (exact f32 products): an exact-f32 FSMN kernel is not built
  if (d.precision == WEKWS_HIP_PRECISION_F32) return generic("precision f32: the any-shape path");
  if (d.num_layers > kFsmnMaxLayers) return generic("deeper than the FSMN kernel's table (16 layers)");
  if (ntaps > kFsmnMaxTaps) return generic("longer memory than the FSMN kernel's taps (32)");
  for (int nt = 1; nt <= kFsmnTileFrames / 16; ++nt)
    if (fsmn_lds_bytes(p.q, 16 * nt, 1) <= kFsmnLdsLimit) p.max_nt = nt;
  if (!p.max_nt) return generic("layer widths beyond the 160 KiB LDS tile");
  p.kind = SHAPE_AS_IS;
  return p;
}
struct FsmnRoute {
  int32_t tile_frames, ntiles;    // the call: cut into tiles of tile_frames, chained through ping-pong workspace caches
  int32_t nt, u;                  // this tile: 16-frame tiles per utterance, utterances per workgroup (nt u <= 4)
  int32_t head_slices, grid, lds_bytes;   // workgroups per tile sharing out_linear2's o-tiles (gridDim.y); gridDim.x; LDS bytes
  size_t ws_bytes, ws_cache;      // the call's scratch: two hand-over caches of ws_cache bytes each (more than one tile)
  const char* why_not;
};
// the route of tile `i` of a call of B utterances x T frames
inline FsmnRoute select_fsmn_route(const FsmnPlan& p, const wekws_hip_desc& d, const RouteOptions& o, int B, int T, int i, int cus) {
  FsmnRoute r{};
  if (p.kind != SHAPE_AS_IS || B <= 0 || T <= 0) { r.why_not = "no FSMN kernel for this model or call"; return r; }
  r.tile_frames = 16 * p.max_nt;
  r.ntiles = (T + r.tile_frames - 1) / r.tile_frames;
  const int P = d.kernel_size + d.stack_size - 1;             // cache frames per layer
  r.ws_cache = size_t(B) * d.num_stack * P * d.num_layers * sizeof(float);
  r.ws_bytes = r.ntiles > 1 ? 2 * r.ws_cache : 0;
  const int Tt = T - i * r.tile_frames < r.tile_frames ? T - i * r.tile_frames : r.tile_frames;
  if (i < 0 || Tt <= 0) { r.why_not = "tile beyond the call"; return r; }
  // short inputs: pack 2 or 4 utterances into one workgroup, as long as every CU still gets a workgroup
  r.nt = (Tt + 15) / 16;
  r.u = 1;
  for (int cand = 4; cand >= 2; cand /= 2)
    if (r.nt * cand <= p.max_nt && r.nt * cand <= 4 && B >= cand * cus && fsmn_lds_bytes(p.q, 16 * r.nt * cand, cand) <= kFsmnLdsLimit) {
      r.u = cand;
      break;
    }
  r.grid = (B + r.u - 1) / r.u;
  // few tiles on many CUs: split the vocabulary-sized last layer over up to 8 workgroups per tile
  r.head_slices = 1;
  if (d.odim >= 256 && r.grid * 2 <= cus) {
    const int sl = cus / r.grid;
    r.head_slices = o.head_slices >= 0 ? (o.head_slices > 0 ? o.head_slices : 1) : (sl > 8 ? 8 : sl);
  }
  r.lds_bytes = fsmn_lds_bytes(p.q, 16 * r.nt * r.u, r.u);
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// wekws_hip_forward_streams: row b of a call continues its stream with frames[b] of the Tcap frames of its row; rows with
// frames[b] <= 0 are skipped.  The plan of a call is
//   STREAMS_DS256    one launch of ds256_stream's table-driven variant, a workgroup per live row;
//   STREAMS_FSMN     one launch of fsmn_f16's table-driven variant: the instance (nt, u) of select_fsmn_route for (live rows,
//                    largest frame count); a workgroup takes up to u rows of EQUAL frame count (a short group leaves slots empty);
//   STREAMS_GROUPED  every other model, and every call whose Tcap exceeds the table-driven kernel's tile: per bucket of rows with
//                    equal frame count a gather from the pool, the uniform forward, a scatter back.
// In every kind the live rows are ordered by frame count, largest first, ties in call order (`order`), and cut into groups
// (`group_start`, ngroups + 1 offsets into `order`; `group_T`): workgroups for the first two kinds, buckets for the third.
enum : int { STREAMS_GROUPED = 0, STREAMS_DS256 = 1, STREAMS_FSMN = 2 };
constexpr int kDs256StreamTile = 16;
struct StreamsPlan {
  int32_t kind, live, max_T, ngroups;
  int32_t slots;                  // rows a group holds at most (STREAMS_FSMN: u; STREAMS_DS256: 1; STREAMS_GROUPED: 0 = any number)
  Route conv;                     // STREAMS_DS256: the kernel instance (grid = live rows)
  FsmnRoute fsmn;                 // STREAMS_FSMN: the kernel instance (grid = ngroups)
  const char* why;                // STREAMS_GROUPED with live rows: why no table-driven kernel takes the call
};
// d / f / o / fp: the model's built-shape descriptor, flags, options and (FSMN) shape plan; plain: the model runs its kernels on
// the caller's own geometry (not zero-padded, not on the any-shape path).  order, group_T: B ints; group_start: B + 1 ints.
inline StreamsPlan plan_streams(const wekws_hip_desc& d, const RouteFlags& f, const RouteOptions& o, const FsmnPlan& fp, bool plain,
                                int cus, int B, int Tcap, const int32_t* frames, int32_t* order, int32_t* group_start, int32_t* group_T) {
  StreamsPlan p{};
  for (int b = 0; b < B; ++b)
    if (frames[b] > 0) {
      order[p.live++] = b;
      p.max_T = frames[b] > p.max_T ? frames[b] : p.max_T;
    }
  std::stable_sort(order, order + p.live, [&](int32_t a, int32_t b) { return frames[a] > frames[b]; });
  group_start[0] = 0;
  if (!p.live) return p;
  const bool conv = d.backbone == WEKWS_HIP_BACKBONE_DS_TCN || d.backbone == WEKWS_HIP_BACKBONE_TCN || d.backbone == WEKWS_HIP_BACKBONE_MDTC;
  if (!plain) p.why = "a zero-padded model or the any-shape path";
  else if (conv) {
    // (the pool's planes are 16-byte aligned; a row whose features are not takes the kernel's own element-wise staging)
    const Route r = select_conv_route(d, f, o, RouteCall{p.live, p.max_T, 1, 1, 1, 1, 1, cus});
    if (r.family != ROUTE_DS256_STREAM) p.why = "no table-driven kernel for this conv model";
    else if (Tcap > kDs256StreamTile) p.why = "rows longer than ds256_stream's tile of 16 frames";
    else { p.kind = STREAMS_DS256; p.conv = r; }
  } else if (d.backbone == WEKWS_HIP_BACKBONE_FSMN) {
    if (select_fsmn_route(fp, d, o, p.live, Tcap, 0, cus).ntiles != 1) p.why = "rows longer than the FSMN kernel's tile";
    else { p.kind = STREAMS_FSMN; p.fsmn = select_fsmn_route(fp, d, o, p.live, p.max_T, 0, cus); }
  } else p.why = "no table-driven GRU kernel";
  p.slots = p.kind == STREAMS_DS256 ? 1 : p.kind == STREAMS_FSMN ? p.fsmn.u : 0;
  for (int i = 0; i < p.live; ++i) {
    const int T = frames[order[i]];
    const bool open = p.ngroups > 0 && group_T[p.ngroups - 1] == T && (!p.slots || i - group_start[p.ngroups - 1] < p.slots);
    if (!open) { group_start[p.ngroups] = i; group_T[p.ngroups++] = T; }
  }
  group_start[p.ngroups] = p.live;
  if (p.kind == STREAMS_DS256) p.conv.grid = p.ngroups;
  if (p.kind == STREAMS_FSMN) p.fsmn.grid = p.ngroups;
  return p;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// What wekws_hip_effective_precision reports for a model that runs the kernels of this file (the any-shape path: exact f32):
// exact f32 where the options or the shape say so; F16 where some call can take a route with one fp16 product (split 0) -- the
// calls at the edges of select_conv_route's choice are asked --; F16X3 otherwise (FSMN: the block-floating kernel).
inline int effective_precision(const wekws_hip_desc& d, const RouteFlags& f, const RouteOptions& o, int cus) {
  if (d.backbone == WEKWS_HIP_BACKBONE_FSMN) return WEKWS_HIP_PRECISION_F16X3;
  if (d.backbone == WEKWS_HIP_BACKBONE_GRU) {
    const int fam = select_gru_route(d, o, GruCall{1, 1, 1, 0, cus}).family;   // (fp16 or not: the same for every call)
    return fam == GRU_F16 || fam == GRU_PIPE ? WEKWS_HIP_PRECISION_F16X3 : WEKWS_HIP_PRECISION_F32;
  }
  if (o.f32) return WEKWS_HIP_PRECISION_F32;
  if (o.split) return WEKWS_HIP_PRECISION_F16X3;
  const int Bs[4] = {1, 2, 3, cus + 1}, Ts[8] = {1, 16, 17, 32, 33, 64, 65, WEKWS_HIP_TILE_FRAMES};
  for (int B : Bs)
    for (int T : Ts)
      for (int bits = 0; bits < 32; ++bits) {
        const RouteCall c{B, T, 1 + (bits & 1), (bits >> 1) & 1, (bits >> 2) & 1, (bits >> 3) & 1, (bits >> 4) & 1, cus};
        const Route r = select_conv_route(d, f, o, c);
        if (r.family != ROUTE_NONE && !r.split) return WEKWS_HIP_PRECISION_F16;
      }
  return WEKWS_HIP_PRECISION_F16X3;
}

}  // namespace wekws
