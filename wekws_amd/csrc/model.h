// The model behind the C ABI (include/wekws_hip.h), as the library's host units share it: the handle types and the host
// functions that cross units.  model.hip: validation, workspaces, destroy, queries; create.hip: packing and upload;
// forward.hip: the forward paths; pool.hip: the stream-cache pool; wekws_hip_hooks.hip: the trace sinks (and, in the test
// library, the debug entry points).
#pragma once

#include <mutex>
#include <vector>

#include "host_util.h"
#include "route.h"
#include "blob_layout.h"
#include "conv_stack.hip.h"
#include "dense_stack_f16.hip.h"
#include "fbank.hip.h"
#include "fsmn_f16.hip.h"
#include "gru_f16.hip.h"
#include "generic.hip.h"

// Scratch device memory of a model, one grow-only buffer per HIP stream that has called it: calls on one stream are
// ordered by the stream, calls on different streams never share a buffer (long-input tile hand-over caches, the
// global head's running sums, the GRU's layer sequences).
struct StreamBuf {
  hipStream_t stream;
  char* ptr;
  size_t bytes;
  char* gran = nullptr;         // GRU wavefront: the granule buffer (gru_pipe.hip.h) -- holds nothing but {data, tag} granules
  size_t gran_bytes = 0;
  unsigned* ctl = nullptr;      // ... and its control words (launch epoch, acknowledgements): allocated ONCE per stream and never
                                // re-allocated -- tags must keep growing for as long as any granule buffer of the stream lives
  unsigned gran_layout = 0;     // how the last wavefront call carved `gran` (slots, layers): a call with another layout clears
                                // it first -- its tag words would otherwise overlay what were DATA words of the old layout
  unsigned* err_h = nullptr;    // one word of pinned, device-mapped HOST memory: a device-side wait that gave up leaves its
  unsigned* err_d = nullptr;    // code here (err_d = the device's address of it); read by the next call, no synchronisation
};

// (block-wise copy between two cache layouts (B, C, P): slice i of the destination -- d_off[i], len[i] -- comes from s_off[i] of the
// source; destination elements outside every slice, or in channels the source does not have, are zero)
struct CacheMap {
  int nb;
  int s_off[wekws::kAmaxMaxBlocks], d_off[wekws::kAmaxMaxBlocks], len[wekws::kAmaxMaxBlocks];
};

struct wekws_hip_model {
  wekws_hip_desc desc;
  int device = 0;
  float* d_w = nullptr;
  wekws::BlockDesc* d_blocks = nullptr;
  wekws::DenseBlock* d_dblocks = nullptr;
  wekws::StackParams sp{};
  wekws::DenseParams dp{};
  // kernel selection (route.h): what the model admits, and the options (defaults = the product choice; wekws_hip_set_option
  // overrides, for A/B measurements and the tests that keep every kernel family parity-green)
  wekws::RouteFlags rf{};
  wekws::RouteOptions ro{};
  float spread_log2 = 0.f;  // Image::spread_log2 of the weights this model was created from
  wekws::GruParams gp{};
  wekws::GruF16Params gq{};
  wekws::FsmnParams fq{};
  wekws::FsmnPlan fplan{};
  int cus = 256;          // compute units of the device (every route's grid)
  // Conv backbones created with a hidden_dim / kernel_size no kernel is built for run as the next built shape (extra channels
  // and the extra OLDEST taps are zero everywhere, see pad_conv_shape); desc then describes the built shape and these keep
  // the caller's: its channel count, its cache length, and how its cache's per-block slices map into the wider ones.
  int user_hdim = 0;
  int user_cache_len = 0;
  CacheMap widen{}, narrow{};
  int cache_len = 0;
  // A shape no specialised kernel is built for (wider / deeper / longer kernels than the reference's recipes use), or an FSMN
  // that must run exact f32: the any-shape path of generic.hip.h on the packer's blob as it is (d_w); nothing else of this
  // struct is used then.
  bool generic = false;
  wekws::GenericModel gm{};
  // Utterances with a NaN / Inf input leave the fast path and are re-computed in exact IEEE f32 (nonfinite.hip.h): the
  // descriptor + packer-order blob the kernels' shape corresponds to, and scratch slots, on the device.
  wekws::NfCtx nf_host{};
  wekws::NfCtx* nf_dev = nullptr;
  float* nf_w = nullptr;
  float* nf_scratch = nullptr;
  unsigned* nf_slots = nullptr;
  std::vector<StreamBuf> ws;       // per-stream workspaces (stream_workspace())
  std::mutex ws_mu;
};

struct wekws_hip_fbank {
  wekws::FbankParams fp{};
  int device = 0;
  float* d_tables = nullptr;
  int resident_f32 = 0, resident_i16 = 0;   // workgroups of one resident round, per sample type (fbank.hip.h)
  int resident_dither_f32 = 0, resident_dither_i16 = 0;   // ... of the dithered kernels (fbank_dither.hip)
};

// ---- model.hip
WEKWS_LOCAL bool desc_conv(const wekws_hip_desc& d);
// validates and returns the blob size (floats: blob_layout.h); 0 with the error text set if invalid
WEKWS_LOCAL size_t blob_elems(const wekws_hip_desc& d);
// -> device pointer to at least `need` bytes owned by (model, stream); nullptr + error text on failure
WEKWS_LOCAL char* stream_workspace(wekws_hip_model* m, hipStream_t stream, size_t need, bool granules = false, unsigned layout = 0);
// the control words of a stream's GRU wavefront launches (gru_pipe.hip.h); nullptr + error text on failure
WEKWS_LOCAL unsigned* stream_ctl(wekws_hip_model* m, hipStream_t stream, unsigned** err_d = nullptr);
// WEKWS_HIP_EDEVICE (once) if a device-side wait of an earlier forward on this stream gave up
WEKWS_LOCAL int stream_health(wekws_hip_model* m, hipStream_t stream);
// frees what a stream's entry owns; true if it held a failure nobody has been told of
WEKWS_LOCAL bool free_stream_buf(StreamBuf& e);

// ---- forward.hip: one forward of (B, T) on the model's device, already current: the backbone's path, then the softmax
WEKWS_LOCAL int forward_call(wekws_hip_model* m, const float* x, int B, int T, const float* in_cache, float* y, float* out_cache,
                             int softmax, hipStream_t stream);

// ---- aux_kernels.hip (gru.hip: launch_conv_nf_fix): the small kernels of the host paths, behind their launch statements (false: the launch failed)
WEKWS_LOCAL void remap_cache(float* dst, const float* src, int B, int Cd, int Pd, int Cs, int Ps, const CacheMap& map, hipStream_t stream);
WEKWS_LOCAL bool launch_conv_nf_fix(const wekws::CallArgs& a, int B, int idim, int cache_elems, hipStream_t stream);
// grouped forward_streams: the rows of a bucket out of their places into (nb, xrow) / (outer, nb, inner), and back
WEKWS_LOCAL bool launch_pool_gather(dim3 grid, const wekws::StreamRow* rows, int nb, float* xg, int xrow, float* cg, int outer, int inner,
                                    hipStream_t stream);
WEKWS_LOCAL bool launch_pool_scatter(dim3 grid, const wekws::StreamRow* rows, int nb, const float* yg, int yrow, const float* cg, int outer,
                                     int inner, hipStream_t stream);

// ---- wekws_hip_hooks.hip: where a forward reports the route of every launch.  Empty in libwekws_hip.so; the test library
// (make hooks) records them for wekws_hip_debug_route_trace / wekws_hip_debug_last_route.
enum : int { kTraceOther = 0, kTraceConv = 1, kTraceAnyShape = 2, kTraceGru = 3, kTraceFsmn = 4, kTraceMaxTiles = 256, kRecInts = 9 };
WEKWS_LOCAL void trace_reset(int path);
WEKWS_LOCAL void trace(int path, const wekws::Route& r);        // (also the thread's last conv route)
WEKWS_LOCAL void trace(int path, const wekws::GruRoute& r);
WEKWS_LOCAL void trace(int path, const wekws::FsmnRoute& r);
