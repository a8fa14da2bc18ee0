// libwekws_hip.so -- C ABI (include/wekws_hip.h) over the gfx950 kernels.
// Host side only: descriptor validation, weight-blob parsing, MFMA fragment pre-packing, upload,
// tiling of long inputs, kernel dispatch.  No torch, no STL types across the boundary.
#include "../../include/wekws_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <optional>
#include <string>
#include <vector>

#include "conv_stack.hip.h"
#include "conv_stack_f16.hip.h"
#include "dense_stack_f16.hip.h"
#include "ds256_w16.hip.h"
#include "ds256_g16.hip.h"
#include "ds256_g32.hip.h"
#include "mdtc64_g4.hip.h"
#include "ds64_g4.hip.h"
#include "ds256_stream.hip.h"
#include "ds256_mm.hip.h"
#include "mdtc64_w16.hip.h"
#include "mdtc64_stream.hip.h"
#include "fbank.hip.h"
#include "fsmn_f16.hip.h"
#include "gru.hip.h"
#include "gru_f16.hip.h"
#include "gru_pipe.hip.h"
#include "generic.hip.h"
#include "route.h"
#include "blob_layout.h"
#include "mfcc.hip.h"
#include "splice.hip.h"
#include "topk.hip.h"
#include "det.hip.h"
#include "weight_image.hip.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

}  // namespace

namespace wekws {
// the thread's last-error message, for entry points defined in other translation units (ctc_kws.hip)
int set_last_error(int code, const char* msg) {
  g_err = msg;
  return code;
}
}  // namespace wekws

namespace {

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return fail(e_ == hipErrorOutOfMemory ? WEKWS_HIP_ENOMEM : WEKWS_HIP_EDEVICE, "%s: %s", \
                  #expr, hipGetErrorString(e_));                                               \
  } while (0)

// Makes `device` current for the scope and restores the caller's device afterwards: the library never changes the
// calling thread's current device behind its back (a Python __del__ may run at any time).
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) ok = hipSetDevice(device) == hipSuccess;
    else prev = -1;                       // already current: nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

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

bool desc_conv(const wekws_hip_desc& d) {
  return d.backbone == WEKWS_HIP_BACKBONE_DS_TCN || d.backbone == WEKWS_HIP_BACKBONE_TCN ||
         d.backbone == WEKWS_HIP_BACKBONE_MDTC;
}

// validates and returns the blob size (floats: blob_layout.h); 0 with g_err set if invalid
size_t blob_elems(const wekws_hip_desc& d) {
  if (d.abi_version != WEKWS_HIP_ABI_VERSION) { fail(WEKWS_HIP_EINVAL, "desc.abi_version %d != %d", d.abi_version, WEKWS_HIP_ABI_VERSION); return 0; }
  if (d.idim <= 0 || d.hdim <= 0 || d.odim <= 0) { fail(WEKWS_HIP_EINVAL, "idim/hdim/odim must be positive"); return 0; }
  if (d.backbone != WEKWS_HIP_BACKBONE_FSMN && (d.aux[0] || d.aux[1])) { fail(WEKWS_HIP_EINVAL, "desc.aux must be 0 for this backbone"); return 0; }
  if (d.precision < 0 || d.precision > WEKWS_HIP_PRECISION_F16) { fail(WEKWS_HIP_EINVAL, "desc.precision %d", d.precision); return 0; }
  if (d.activation < 0 || d.activation > WEKWS_HIP_ACT_SOFTMAX) { fail(WEKWS_HIP_EINVAL, "desc.activation %d", d.activation); return 0; }
  if (d.activation == WEKWS_HIP_ACT_SOFTMAX && (d.head == WEKWS_HIP_HEAD_GLOBAL || d.head == WEKWS_HIP_HEAD_LAST)) {
    fail(WEKWS_HIP_EINVAL, "softmax activation needs a per-frame head (forward_softmax is softmax over axis 2)");
    return 0;
  }
  if (d.backbone == WEKWS_HIP_BACKBONE_FSMN) {
    if (d.num_layers <= 0 || d.num_stack <= 0 || d.kernel_size <= 0 || d.stack_size <= 0 || d.aux[0] <= 0 || d.aux[1] <= 0) {
      fail(WEKWS_HIP_EINVAL, "fsmn: num_layers/proj_dim/left_order/right_order/affine dims must be positive");
      return 0;
    }
    if (d.head != WEKWS_HIP_HEAD_IDENTITY || d.activation == WEKWS_HIP_ACT_SIGMOID || d.preproc_relu) {
      fail(WEKWS_HIP_EINVAL, "fsmn: preprocessing none, identity classifier and identity activation only");
      return 0;
    }
    return size_t(wekws::blob_layout(d).total);
  }
  switch (d.backbone) {
    case WEKWS_HIP_BACKBONE_DS_TCN:
    case WEKWS_HIP_BACKBONE_TCN:
      if (d.num_layers <= 0 || d.kernel_size <= 0) { fail(WEKWS_HIP_EINVAL, "tcn: num_layers/kernel_size"); return 0; }
      break;
    case WEKWS_HIP_BACKBONE_MDTC:
      if (d.num_stack <= 0 || d.stack_size <= 0 || d.kernel_size <= 0) { fail(WEKWS_HIP_EINVAL, "mdtc: num_stack/stack_size/kernel_size"); return 0; }
      break;
    case WEKWS_HIP_BACKBONE_GRU:
      if (d.num_layers <= 0) { fail(WEKWS_HIP_EINVAL, "gru: num_layers"); return 0; }
      break;
    default:
      fail(WEKWS_HIP_EINVAL, "unknown backbone %d", d.backbone);
      return 0;
  }
  switch (d.head) {
    case WEKWS_HIP_HEAD_LINEAR: break;
    case WEKWS_HIP_HEAD_GLOBAL:
    case WEKWS_HIP_HEAD_LAST:
      if (d.head_hidden <= 0) { fail(WEKWS_HIP_EINVAL, "head_hidden must be positive"); return 0; }
      break;
    case WEKWS_HIP_HEAD_IDENTITY:
      if (d.odim != d.hdim) { fail(WEKWS_HIP_EINVAL, "identity head needs odim == hdim"); return 0; }
      break;
    default:
      fail(WEKWS_HIP_EINVAL, "unknown head %d", d.head);
      return 0;
  }
  return size_t(wekws::blob_layout(d).total);   // blob_layout.h: the one statement of the layout
}

}  // namespace

// (block-wise copy between two cache layouts (B, C, P): slice i of the destination -- d_off[i], len[i] -- comes from s_off[i] of the
// source; destination elements outside every slice, or in channels the source does not have, are zero)
struct CacheMap {
  int nb;
  int s_off[wekws::kAmaxMaxBlocks], d_off[wekws::kAmaxMaxBlocks], len[wekws::kAmaxMaxBlocks];
};
static __global__ void cache_remap_kernel(float* __restrict__ dst, const float* __restrict__ src, int B, int Cd, int Pd, int Cs, int Ps,
                                          const CacheMap m) {
  const int64_t n = int64_t(B) * Cd * Pd;
  for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < n; e += int64_t(gridDim.x) * blockDim.x) {
    const int p = int(e % Pd);
    const int64_t bc = e / Pd;
    const int c = int(bc % Cd), b = int(bc / Cd);
    float v = 0.f;
    if (c < Cs) {
      for (int i = 0; i < m.nb; ++i)
        if (p >= m.d_off[i] && p < m.d_off[i] + m.len[i]) v = src[(int64_t(b) * Cs + c) * Ps + m.s_off[i] + (p - m.d_off[i])];
    }
    dst[e] = v;
  }
}
static void remap_cache(float* dst, const float* src, int B, int Cd, int Pd, int Cs, int Ps, const CacheMap& map, hipStream_t stream) {
  const int grid = int(std::min<size_t>((size_t(B) * Cd * Pd + 255) / 256, 4096));
  hipLaunchKernelGGL(cache_remap_kernel, dim3(grid), dim3(256), 0, stream, dst, src, B, Cd, Pd, Cs, Ps, map);
}

// The same re-computation as its own launch, behind a kernel that is left exactly as it was (the register-resident kernels of
// ds64_g4.hip.h / mdtc64_g4.hip.h: one utterance per small workgroup, several workgroups per CU, at the register limit -- a
// detection branch inside them moved their register allocation into scratch).  One workgroup per utterance: a pass over its
// features (and incoming cache); what the kernel before wrote for an utterance with a NaN / Inf input is overwritten.
static __global__ __launch_bounds__(256) void conv_nf_fix_kernel(const wekws::CallArgs A, int idim, int cache_elems) {
  __shared__ unsigned cell;
  const int b = blockIdx.x;
  bool bad = wekws::nf_scan_rows(A.x + int64_t(b) * A.xs_b, A.T, idim, idim, &cell);
  if (!bad && A.in_cache) bad = wekws::nf_scan(A.in_cache + int64_t(b) * cache_elems, cache_elems, &cell);
  if (bad) wekws::nf_repair_call(A, b);
}

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

// NoSubsampling (subsampling.py:35-36) arrives as a square preprocessing matrix that is diagonal (the packer folds a CMVN into it)
static bool pre_is_diagonal(const wekws_hip_desc& d, const float* blob) {
  if (d.backbone == WEKWS_HIP_BACKBONE_FSMN || d.idim != d.hdim) return false;
  for (int r = 0; r < d.hdim; ++r)
    for (int k = 0; k < d.idim; ++k)
      if (r != k && blob[size_t(r) * d.idim + k] != 0.f) return false;
  return true;
}

// (measurement aid: WEKWS_NF_FIX_ALL=1 runs the separate non-finite pass behind EVERY conv kernel, to price the extra launch)
static bool nf_fix_all() {
  static const bool v = [] { const char* e = std::getenv("WEKWS_NF_FIX_ALL"); return e && e[0] == '1'; }();
  return v;
}
static thread_local wekws::Route g_last_route{};             // the route of this thread's last conv launch (tests: hooks build)
// the route of EVERY tile of this thread's last forward (wekws_hip_debug_route_trace; hooks build only), as records of 9 ints
enum : int { kTraceOther = 0, kTraceConv = 1, kTraceAnyShape = 2, kTraceGru = 3, kTraceFsmn = 4, kTraceMaxTiles = 256, kRecInts = 9 };

// The device-side context of nonfinite.hip.h for a model whose kernels run shape `d` on packer-order blob `blob` (host).
// tmax: most frames one kernel call covers.  Returns a WEKWS_HIP_* code.
static int nf_setup(wekws_hip_model* m, const wekws_hip_desc& d, const float* blob, size_t n_elems, int tmax) {
  wekws::NfCtx& c = m->nf_host;
  c = wekws::NfCtx{};
  c.d = d;
  c.nslots = 16;
  c.skip_zero = 0;
  c.tmax = tmax;
  int64_t slot = 0;
  if (d.backbone == WEKWS_HIP_BACKBONE_GRU) {
    c.width = d.hdim;
    slot = int64_t(d.num_layers) * d.hdim + 7 * int64_t(d.hdim);
  } else if (d.backbone == WEKWS_HIP_BACKBONE_FSMN) {
    c.cache_len = d.kernel_size - 1 + d.stack_size;
    c.pmax = c.cache_len;
    c.width = std::max(std::max(d.hdim, d.num_stack), std::max(d.aux[0], d.aux[1]));
    slot = 4 * int64_t(tmax) * c.width + int64_t(c.pmax + tmax) * d.num_stack;
  } else {
    const wekws::ConvSchedule s = wekws::conv_schedule(d);
    c.cache_len = int(s.cache_len);
    c.pmax = s.max_pad;
    c.width = std::max(d.hdim, d.head_hidden);
    slot = 4 * int64_t(tmax) * c.width + int64_t(c.pmax + tmax) * d.hdim;
  }
  c.slot_floats = (slot + 63) / 64 * 64;
  c.pre_diag = pre_is_diagonal(d, blob);
  hipError_t e = hipMalloc(&m->nf_w, n_elems * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(m->nf_w, blob, n_elems * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&m->nf_scratch, size_t(c.slot_floats) * c.nslots * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&m->nf_slots, c.nslots * sizeof(unsigned));
  if (e == hipSuccess) e = hipMemset(m->nf_slots, 0, c.nslots * sizeof(unsigned));
  if (e == hipSuccess) e = hipMalloc(&m->nf_dev, sizeof(wekws::NfCtx));
  c.w = m->nf_w;
  c.scratch = m->nf_scratch;
  c.slots = m->nf_slots;
  if (e == hipSuccess) e = hipMemcpy(m->nf_dev, &c, sizeof(c), hipMemcpyHostToDevice);
  if (e != hipSuccess)
    return fail(e == hipErrorOutOfMemory ? WEKWS_HIP_ENOMEM : WEKWS_HIP_EDEVICE, "non-finite path setup: %s", hipGetErrorString(e));
  return WEKWS_HIP_OK;
}
static void nf_teardown(wekws_hip_model* m) {
  if (m->nf_w) (void)hipFree(m->nf_w);
  if (m->nf_scratch) (void)hipFree(m->nf_scratch);
  if (m->nf_slots) (void)hipFree(m->nf_slots);
  if (m->nf_dev) (void)hipFree(m->nf_dev);
  m->nf_w = m->nf_scratch = nullptr;
  m->nf_slots = nullptr;
  m->nf_dev = nullptr;
}
// a zero-padded model (pad_conv_shape / pad_gru_hidden): zero weights contribute nothing on the non-finite path
static int nf_set_skip_zero(wekws_hip_model* m) {
  m->nf_host.skip_zero = 1;
  if (!m->nf_dev) return WEKWS_HIP_OK;
  DeviceGuard guard(m->device);
  if (hipMemcpy(m->nf_dev, &m->nf_host, sizeof(m->nf_host), hipMemcpyHostToDevice) != hipSuccess)
    return fail(WEKWS_HIP_EDEVICE, "non-finite path setup (padded model)");
  return WEKWS_HIP_OK;
}

// the stream's entry of m->ws, added on its first call (the caller holds ws_mu)
static StreamBuf* stream_buf(wekws_hip_model* m, hipStream_t stream) {
  for (auto& e : m->ws) if (e.stream == stream) return &e;
  m->ws.push_back(StreamBuf{stream, nullptr, 0});
  return &m->ws.back();
}
// frees what a stream's entry owns; true if it held a failure nobody has been told of (the device memory first: hipFree waits for
// the work that may still use it -- the caller's stream handles are not touched, they may have been destroyed before the model -- so
// the health word is final when it is read)
static bool free_stream_buf(StreamBuf& e) {
  if (e.ptr) (void)hipFree(e.ptr);
  if (e.gran) (void)hipFree(e.gran);
  if (e.ctl) (void)hipFree(e.ctl);
  const bool gave_up = e.err_h && *static_cast<volatile unsigned*>(e.err_h) != 0u;
  if (e.err_h) (void)hipHostFree(e.err_h);
  return gave_up;
}
// -> device pointer to at least `need` bytes owned by (model, stream); nullptr + error text on failure
static char* stream_workspace(wekws_hip_model* m, hipStream_t stream, size_t need, bool granules = false, unsigned layout = 0) {
  std::lock_guard<std::mutex> lk(m->ws_mu);
  StreamBuf* sb = stream_buf(m, stream);
  char*& ptr = granules ? sb->gran : sb->ptr;
  size_t& bytes = granules ? sb->gran_bytes : sb->bytes;
  if (bytes < need) {
    // Growing frees the old buffer behind a stream synchronisation -- which a stream that is being captured into a HIP
    // graph cannot do: such a call fails and names wekws_hip_reserve (no hidden synchronisation inside a capture).
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
      fail(WEKWS_HIP_EINVAL, "this call needs %zu bytes of workspace on a stream that is being captured: call "
                             "wekws_hip_reserve(model, B, T, stream) before the capture begins", need);
      return nullptr;
    }
    if (ptr) {
      (void)hipStreamSynchronize(stream);                     // earlier calls on this stream may still use the old buffer
      (void)hipFree(ptr);
      ptr = nullptr; bytes = 0;
    }
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&ptr), need);
    if (e != hipSuccess) {
      ptr = nullptr;
      fail(e == hipErrorOutOfMemory ? WEKWS_HIP_ENOMEM : WEKWS_HIP_EDEVICE, "workspace of %zu bytes: %s", need, hipGetErrorString(e));
      return nullptr;
    }
    bytes = need;
    // GRU wavefront (gru_pipe.hip.h): a granule buffer must never show a word that was not written as a tag -- it is
    // cleared once, here (tags start at 1 and only grow: the epoch lives in StreamBuf::ctl, which is never re-allocated)
    if (granules && hipMemsetAsync(ptr, 0, need, stream) != hipSuccess) {
      fail(WEKWS_HIP_EDEVICE, "workspace: hipMemsetAsync");
      return nullptr;
    }
    if (granules) sb->gran_layout = layout;
  }
  // ... and again whenever a call carves the buffer differently from the call before it (another number of slots): gate
  // granules carry their tag in every fourth word, state granules in every second, so a tag position of the new layout may
  // hold a float of the old one -- which after days of streaming could equal a live tag.  Stream-ordered, no synchronisation.
  if (granules && layout && sb->gran_layout != layout) {
    if (sb->gran_layout && hipMemsetAsync(ptr, 0, bytes, stream) != hipSuccess) {
      fail(WEKWS_HIP_EDEVICE, "workspace: hipMemsetAsync");
      return nullptr;
    }
    sb->gran_layout = layout;
  }
  return ptr;
}

// The control words of a stream's GRU wavefront launches (gru_pipe.hip.h): one small allocation per (model, stream), made
// on the first call (or by wekws_hip_reserve) and kept until the stream's workspace is released.
static unsigned* stream_ctl(wekws_hip_model* m, hipStream_t stream, unsigned** err_d = nullptr) {
  std::lock_guard<std::mutex> lk(m->ws_mu);
  StreamBuf* sb = stream_buf(m, stream);
  if (!sb->ctl) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
      fail(WEKWS_HIP_EINVAL, "first GRU call on a stream that is being captured: call wekws_hip_reserve(model, B, T, stream) before the capture begins");
      return nullptr;
    }
    if (hipMalloc(reinterpret_cast<void**>(&sb->ctl), wekws::kGruPipeCtlBytes) != hipSuccess ||
        hipMemsetAsync(sb->ctl, 0, wekws::kGruPipeCtlBytes, stream) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&sb->err_h), 64, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&sb->err_d), sb->err_h, 0) != hipSuccess) {
      if (sb->ctl) (void)hipFree(sb->ctl);
      if (sb->err_h) (void)hipHostFree(sb->err_h);
      sb->ctl = nullptr;
      sb->err_h = sb->err_d = nullptr;
      fail(WEKWS_HIP_ENOMEM, "GRU control words");
      return nullptr;
    }
    *static_cast<volatile unsigned*>(sb->err_h) = 0u;
  }
  if (err_d) *err_d = sb->err_d;
  return sb->ctl;
}

// Has a device-side wait of an earlier forward on this stream given up (gru_pipe.hip.h: give_up)?  Reads the stream's word of
// host memory -- no device call on the healthy path --; if set, clears it (host word now, the device's copy in stream order)
// and returns WEKWS_HIP_EDEVICE with the stage named.  The word is written by the kernel itself, so a caller that pipelines
// forwards hears of a failure on the first call AFTER the failed launch has run, at the latest from wekws_hip_forward_status.
static int stream_health(wekws_hip_model* m, hipStream_t stream) {
  unsigned* err_h = nullptr;
  unsigned* ctl = nullptr;
  {
    std::lock_guard<std::mutex> lk(m->ws_mu);
    for (auto& e : m->ws) if (e.stream == stream) { err_h = e.err_h; ctl = e.ctl; }
  }
  if (!err_h) return WEKWS_HIP_OK;
  const unsigned code = *static_cast<volatile unsigned*>(err_h);
  if (!code) return WEKWS_HIP_OK;
  // The host word is cleared only once the clear of the DEVICE word is really queued behind the launches that saw it (stream
  // order): launches already queued behind the failed one still find the device word set, end at once and set the host word
  // again -- the next call reports them too.  During a capture (or if the memset cannot be queued) both words stay: every call
  // keeps failing until a call outside the capture can clear them.
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
  if (ctl && !capturing && hipMemsetAsync(ctl + 2, 0, sizeof(unsigned), stream) == hipSuccess)
    *static_cast<volatile unsigned*>(err_h) = 0u;
  return fail(WEKWS_HIP_EDEVICE, "a bounded wait of the GRU wavefront gave up (code 0x%x: %s of stage %u): the outputs of the "
              "forwards issued on this stream since the last successful call -- including calls that returned OK while "
              "the failed launch was still queued -- are not valid", code,
              (code >> 8) == 1 ? "data" : "credit", code & 0xffu);
}

struct wekws_hip_fbank {
  wekws::FbankParams fp{};
  int device = 0;
  float* d_tables = nullptr;
  int resident_f32 = 0, resident_i16 = 0;   // workgroups of one resident round, per sample type (fbank.hip.h)
};

#ifdef WEKWS_TEST_HOOKS   // libwekws_hip_hooks.so only (make hooks)
#include "wekws_hip_hooks.hip.h"
#else
template <class R>
static void trace(int, const R&) {}
static void trace_reset(int) {}
#endif

// The start of every create path: the device checked and made current for the caller's scope (guard), the model allocated, its
// compute units counted.
static int open_model(int device, const wekws_hip_desc& d, std::optional<DeviceGuard>& guard, wekws_hip_model** out) {
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(WEKWS_HIP_EDEVICE, "device %d of %d", device, ndev);
  guard.emplace(device);
  if (!guard->ok) return fail(WEKWS_HIP_EDEVICE, "hipSetDevice(%d)", device);
  wekws_hip_model* m = new (std::nothrow) wekws_hip_model();
  if (!m) return fail(WEKWS_HIP_ENOMEM, "host allocation");
  m->desc = d;
  m->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) m->cus = prop.multiProcessorCount;
  *out = m;
  return WEKWS_HIP_OK;
}
// `bytes` of host data as a device allocation in *dst; a failure destroys the model (what it owns so far with it)
template <class T>
static int upload_or_destroy(wekws_hip_model* m, T** dst, const void* src, size_t bytes) {
  hipError_t e = hipMalloc(reinterpret_cast<void**>(dst), bytes);
  if (e == hipSuccess) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) return WEKWS_HIP_OK;
  wekws_hip_destroy(m);
  return fail(e == hipErrorOutOfMemory ? WEKWS_HIP_ENOMEM : WEKWS_HIP_EDEVICE, "weight upload: %s", hipGetErrorString(e));
}

// A valid reference configuration without a specialised kernel (`why` names the limit it exceeds): the any-shape exact-f32
// path (generic.hip.h).  The reference's init_model takes any size (kws_model.py:114-170); before round 5 these were
// WEKWS_HIP_EUNSUPPORTED.
static int create_generic(const wekws_hip_desc& d, const float* blob, size_t n_elems, int device, wekws_hip_model** out) {
  if (desc_conv(d)) {
    // dilations are powers of two of the depth and the cache length is their sum times (kernel_size - 1): a corrupt descriptor
    // (hundreds of layers) must not reach the shift or overflow the int the kernels index with
    const int depth = d.backbone == WEKWS_HIP_BACKBONE_MDTC ? d.stack_size : d.num_layers;
    if (depth > 24) return fail(WEKWS_HIP_EINVAL, "dilation 2^%d: %d layers per stack is beyond any receptive field", depth - 1, depth);
    const int64_t sum = wekws::conv_schedule(d).cache_len;
    if (sum * std::max(1, d.hdim) > int64_t(INT32_MAX) / 4)
      return fail(WEKWS_HIP_EINVAL, "cache of %lld frames x %d channels per stream is out of range", (long long)sum, d.hdim);
  }
  std::optional<DeviceGuard> guard;
  wekws_hip_model* m = nullptr;
  if (const int rc = open_model(device, d, guard, &m); rc != WEKWS_HIP_OK) return rc;
  m->generic = true;
  m->ro.gru_pipe = 0;
  if (const int rc = upload_or_destroy(m, &m->d_w, blob, n_elems * sizeof(float)); rc != WEKWS_HIP_OK) return rc;
  m->gm.d = d;
  m->gm.w = m->d_w;
  m->gm.pre_diag = pre_is_diagonal(d, blob);
  m->gm.cache_len = m->cache_len = wekws::gen_cache_len(d);
  *out = m;
  return WEKWS_HIP_OK;
}

// FSMN: validate (blob_elems), zero-pad every channel count to a multiple of 32, pre-split + pre-pack the six kinds of dense
// layers as MFMA A operands (fsmn_f16.hip.h), upload.
static int create_fsmn(const wekws_hip_desc& d, const float* blob_in, size_t n_elems, int device, wekws_hip_model** out) {
  // every precision request but F32 is served by the block-floating split-fp16 kernel (22-bit products, fp32 accumulate: the
  // accuracy of fp32 arithmetic at any operand scale, tests/test_hip_parity.py::test_scale_sweep); F32, and shapes beyond the
  // kernel's tables or LDS: the any-shape path (route.h: fsmn_shape_plan)
  const wekws::FsmnPlan plan = wekws::fsmn_shape_plan(d);
  if (plan.kind == wekws::SHAPE_GENERIC) return create_generic(d, blob_in, n_elems, device, out);
  std::vector<float> balanced(blob_in, blob_in + n_elems);
  balance_operand_channels(d, balanced.data());
  const float* blob = balanced.data();
  const int I = d.idim, D = d.num_stack, K = d.odim;
  const int ntaps = d.kernel_size + d.stack_size;
  wekws::FsmnParams q{};
  q.idim = I; q.odim = K; q.proj = D;
  q.kin = plan.q.kin; q.a1p = plan.q.a1p; q.linp = plan.q.linp; q.dp = plan.q.dp; q.a2p = plan.q.a2p; q.op = plan.q.op;
  q.nlayers = d.num_layers; q.ntaps = ntaps; q.P = ntaps - 1; q.taps_ld = plan.q.taps_ld;

  Image img;
  img.reserve(4);
  const wekws::BlobLayout L = wekws::blob_layout(d);
  // a dense layer W[O][Ksrc] (+ bias[O], or none): A operand padded to (Op x Kp); bias padded with zeros to Op
  // block floating point (fsmn_f16.hip.h): matrix scale, and the output bound |W a + b| <= alpha max|a| + beta
  auto dense = [&](const wekws::BlobTensor& w, const wekws::BlobTensor* b, int Op, uint32_t* a_off, uint32_t* b_off, wekws::FsmnDense* fd) {
    const int O = int(w.rows), Ksrc = w.cols;
    const float* W = blob + w.off;
    std::vector<float> wp(size_t(Op) * Ksrc, 0.f);
    std::memcpy(wp.data(), W, size_t(O) * Ksrc * sizeof(float));
    *a_off = img.put_packed_a16(wp.data(), Op, Ksrc, Ksrc, &fd->inv_s);
    // (1.0001: summation order / rounding of the device's accumulation)
    l1_bound<double>(W, O, Ksrc, Ksrc, b ? blob + b->off : nullptr, 1.0001f, &fd->alpha, &fd->beta);
    if (b) {
      std::vector<float> bp(Op, 0.f);
      std::memcpy(bp.data(), blob + b->off, size_t(O) * sizeof(float));
      *b_off = img.put(bp.data(), Op);
    }
  };
  dense(L.in1_w(), &L.in1_b(), q.a1p, &q.in1_a, &q.in1_b, &q.in1);
  dense(L.in2_w(), &L.in2_b(), q.linp, &q.in2_a, &q.in2_b, &q.in2);
  for (int l = 0; l < d.num_layers; ++l) {
    const wekws::FsmnWeights lw = L.fsmn_layer(l);
    const float* taps = blob + lw.taps.off;
    dense(lw.wproj, nullptr, q.dp, &q.layer[l].wp_a, nullptr, &q.layer[l].wp);
    std::vector<float> tp(size_t(q.dp) * q.taps_ld, 0.f);
    for (int c = 0; c < D; ++c) std::memcpy(&tp[size_t(c) * q.taps_ld], taps + size_t(c) * ntaps, ntaps * sizeof(float));
    float no_bias;
    l1_bound<float>(taps, D, ntaps, ntaps, nullptr, 1.00001f, &q.layer[l].taps_l1, &no_bias);
    q.layer[l].taps = img.put(tp.data(), tp.size());
    dense(lw.waff, &lw.baff, q.linp, &q.layer[l].wa_a, &q.layer[l].wa_b, &q.layer[l].wa);
  }
  dense(L.out1_w(), &L.out1_b(), q.a2p, &q.out1_a, &q.out1_b, &q.out1);
  dense(L.out2_w(), &L.out2_b(), q.op, &q.out2_a, &q.out2_b, &q.out2);
  if (img.spread_log2 > WEKWS_HIP_F16X3_ENVELOPE_LOG2) {
    // a weight matrix spreads its row / column magnitudes beyond the envelope in which the split-fp16 kernel keeps fp32-level
    // accuracy: exact f32 instead (wekws_hip_effective_precision reports F32, wekws_hip_weight_spread_log2 the spread)
    const float spread = img.spread_log2;
    const int rc = create_generic(d, blob_in, n_elems, device, out);
    if (rc == WEKWS_HIP_OK) { (*out)->spread_log2 = spread; (*out)->rf.out_of_envelope = true; }
    return rc;
  }

  std::optional<DeviceGuard> guard;
  wekws_hip_model* m = nullptr;
  if (const int rc = open_model(device, d, guard, &m); rc != WEKWS_HIP_OK) return rc;
  m->cache_len = q.P;
  m->fplan = plan;
  m->ro = wekws::route_defaults(d, m->rf);
  if (const int rc = upload_or_destroy(m, &m->d_w, img.data.data(), img.data.size() * sizeof(float)); rc != WEKWS_HIP_OK) return rc;
  q.w = m->d_w;
  m->fq = q;
  m->spread_log2 = img.spread_log2;
  if (const int rc = nf_setup(m, d, blob_in, n_elems, 16 * plan.max_nt); rc != WEKWS_HIP_OK) {
    wekws_hip_destroy(m);
    return rc;
  }
  *out = m;
  return WEKWS_HIP_OK;
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
    hipLaunchKernelGGL(wekws::gru_nf_fix_kernel, dim3(B), dim3(256), 0, stream, m->nf_dev, x, B, T, in_cache, out_cache, y);
    if (hipGetLastError() != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "gru non-finite pass: launch failed");
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
  const bool per_frame = d.head == WEKWS_HIP_HEAD_LINEAR || d.head == WEKWS_HIP_HEAD_IDENTITY;
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
    g_last_route = route;
    trace(kTraceConv, route);
    a.head_slices = route.head_slices;
    const int rc = launch_conv_route(route, m, a, stream);
    // (a launcher that refuses what the route chose: the two have drifted apart -- an internal error, never a silent fall-through)
    if (rc == -4)
      return fail(WEKWS_HIP_EUNSUPPORTED, "internal: kernel family %s has no kernel for the route (C=%d nt=%d T=%d cache %d/%d threads %d LDS %d)",
                  wekws::route_family_name(route.family), C, route.nt, Tt, rcall.has_in, rcall.has_out, route.threads, route.lds_bytes);
    if (rc) return fail(rc, "conv-stack launch failed (C=%d nt=%d): %s", C, route.nt, hipGetErrorString(hipGetLastError()));
    if (nf_fix_all()) {                                    // (measurement aid only: the non-finite pass as its own launch)
      hipLaunchKernelGGL(conv_nf_fix_kernel, dim3(B), dim3(256), 0, stream, a, d.idim, C * m->cache_len);
      if (hipGetLastError() != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "non-finite pass: launch failed");
    }
  }
  if (user_out_cache) remap_cache(user_out_cache, out_cache, B, m->user_hdim, m->user_cache_len, C, m->cache_len, m->narrow, stream);
  return WEKWS_HIP_OK;
}

// A shape no kernel is built for, run as the next built one (plan: route.h), zero-padded -- exact, see pad_conv_shape / pad_gru_hidden:
// conv backbones of any width up to 256 and any kernel size up to the built one (kws_model.py:114,142-157 take any), GRUs below the
// built hidden size.  The model is the built shape's; it keeps the caller's channel count and how the caller's cache maps into its own.
static int create_padded(const wekws_hip_desc& d, const wekws::ShapePlan& plan, const float* blob, int device, wekws_hip_model** out) {
  const bool conv = desc_conv(d);
  wekws_hip_desc dd = d;
  dd.hdim = plan.C;
  if (conv) dd.kernel_size = plan.ks;
  const std::vector<float> wide = conv ? pad_conv_shape(d, blob, dd) : pad_gru_hidden(d, blob, dd);
  if (wide.size() != blob_elems(dd)) return fail(WEKWS_HIP_EINVAL, "internal: widened blob has %zu floats, expected %zu", wide.size(), blob_elems(dd));
  const int rc = wekws_hip_create(&dd, wide.data(), wide.size(), device, out);
  if (rc != WEKWS_HIP_OK) return rc;
  wekws_hip_model* m = *out;
  m->user_hdim = d.hdim;
  if (const int rz = nf_set_skip_zero(m); rz != WEKWS_HIP_OK) { wekws_hip_destroy(m); *out = nullptr; return rz; }
  if (!conv) {
    m->widen.nb = m->narrow.nb = 1;                          // states (L, B, H): one "slice" per row
    m->widen.s_off[0] = m->widen.d_off[0] = m->narrow.s_off[0] = m->narrow.d_off[0] = 0;
    m->widen.len[0] = m->narrow.len[0] = d.hdim;
    return WEKWS_HIP_OK;
  }
  // the caller's cache: per block (ks - 1) dil frames, the tail of the built kernel's (ks_built - 1) dil
  const wekws::ConvSchedule user = wekws::conv_schedule(d), built = wekws::conv_schedule(dd);
  m->widen.nb = m->narrow.nb = user.nb;
  for (int i = 0; i < user.nb; ++i) {
    const wekws::ConvBlock u = user.block(i), b = built.block(i);
    m->widen.s_off[i] = m->narrow.d_off[i] = u.cache_off;
    m->widen.d_off[i] = m->narrow.s_off[i] = b.cache_off + (b.pad - u.pad);
    m->widen.len[i] = m->narrow.len[i] = u.pad;
  }
  m->user_cache_len = int(user.cache_len);
  return WEKWS_HIP_OK;
}

// The weight image of a conv model (preprocessing, residual blocks, classifier) and the kernels' parameters and block tables;
// every tensor from where blob_layout.h says it lies.
static void pack_conv(const wekws_hip_desc& d, const float* blob, Image& img, wekws_hip_model* m,
                      std::vector<wekws::BlockDesc>& blocks, std::vector<wekws::DenseBlock>& dblocks) {
  const int C = d.hdim, ks = d.kernel_size, K = d.odim;
  const wekws::BlobLayout L = wekws::blob_layout(d);
  wekws::StackParams& sp = m->sp;
  sp.pre_a = img.put_packed_a(blob + L.pre_w().off, C, d.idim, d.idim);
  sp.pre_inv_s = 1.f;
  sp.pre_a16 = img.put_packed_a16(blob + L.pre_w().off, C, d.idim, d.idim, &sp.pre_inv_s);
  sp.pre_b = img.put(blob + L.pre_b().off, C);
  sp.idim = d.idim;
  sp.kpre = round_up(d.idim, 16);
  sp.ksize = ks;
  sp.odim = K;
  sp.pre_relu = d.preproc_relu;
  sp.kpre16 = round_up(d.idim, 32);
  sp.head_inv_s = 1.f;
  const wekws::ConvSchedule sched = wekws::conv_schedule(d);
  for (int i = 0; i < sched.nb; ++i) {
    const wekws::ConvBlock cb = sched.block(i);
    const wekws::ConvWeights bw = L.block(i);
    const float *wd = blob + bw.wd.off, *bd = blob + bw.bd.off, *w1 = blob + bw.w1.off, *b1 = blob + bw.b1.off;
    wekws::BlockDesc b{};
    b.inv_s1 = b.inv_s2 = b.dw_tap_s = b.dw_tap_inv = 1.f;
    b.dil = cb.dil; b.pad = cb.pad; b.cache_off = cb.cache_off; b.zadd = cb.zadd;
    wekws::DenseBlock db{};
    db.dil = b.dil; db.pad = b.pad; db.cache_off = b.cache_off; db.zadd = b.zadd; db.inv_s1 = 1.f;
    if (d.backbone == WEKWS_HIP_BACKBONE_TCN) {
      b.a1 = img.put_packed_a(w1, C, C * ks, C * ks);
      b.a1_16 = img.put_packed_a16(w1, C, C * ks, C * ks, &b.inv_s1);
      {  // dense-stack kernel: K reordered to (tap, channel)
        std::vector<float> mw(size_t(C) * C * ks);
        for (int o = 0; o < C; ++o)
          for (int c = 0; c < C; ++c)
            for (int j = 0; j < ks; ++j) mw[(size_t(o) * ks + j) * C + c] = w1[(size_t(o) * C + c) * ks + j];
        db.a1 = img.put_packed_a16(mw.data(), C, C * ks, C * ks, &db.inv_s1);
      }
      b.b1 = img.put(b1, C);
      db.b1 = b.b1;
    } else {
      b.dw_w = img.put(wd, size_t(C) * ks);
      b.dw_b = img.put(bd, C);
      {  // taps + bias of a channel side by side, padded to whole float4s (one or three 16-byte loads per row)
        const int dwp = round_up(ks + 1, 4);
        std::vector<float> pk(size_t(C) * dwp, 0.f);
        for (int c = 0; c < C; ++c) {
          for (int j = 0; j < ks; ++j) pk[size_t(c) * dwp + j] = wd[size_t(c) * ks + j];
          pk[size_t(c) * dwp + ks] = bd[c];
        }
        b.dw_pk = img.put(pk.data(), pk.size());
      }
      // block floating point: the depthwise output obeys |dw(u) + b| <= dw_alpha * max|u| + dw_beta (1.0000005: rounding of the
      // tap sum and of the device's FMA chain); the taps enter the matrix cores (ds256_mm) scaled to the top of the fp16 range
      l1_bound<float>(wd, C, ks, ks, bd, 1.0000005f, &b.dw_alpha, &b.dw_beta);
      float tmax = 0.f;
      for (size_t e = 0; e < size_t(C) * ks; ++e)
        if (std::isfinite(wd[e]) && std::fabs(wd[e]) > tmax) tmax = std::fabs(wd[e]);
      b.dw_tap_s = pow2_scale_host(tmax, &b.dw_tap_inv);
      b.a1 = img.put_packed_a(w1, C, C, C);
      b.a1_16 = img.put_packed_a16(w1, C, C, C, &b.inv_s1);
      // |W1 a + b1| <= mid_alpha * max|a| + mid_beta (MDTC mid tile)
      l1_bound<float>(w1, C, C, C, b1, 1.0001f, &b.mid_alpha, &b.mid_beta);
      b.b1 = img.put(b1, C);
      if (d.backbone == WEKWS_HIP_BACKBONE_MDTC) {
        b.a2 = img.put_packed_a(blob + bw.w2.off, C, C, C);
        b.a2_16 = img.put_packed_a16(blob + bw.w2.off, C, C, C, &b.inv_s2);
        b.b2 = img.put(blob + bw.b2.off, C);
      }
    }
    blocks.push_back(b);
    dblocks.push_back(db);
  }
  const int off = int(sched.cache_len);
  m->cache_len = off;
  sp.cache_len = off;
  sp.nblocks = sched.nb;
  sp.head = d.head;
  sp.head_hidden = d.head_hidden;
  sp.sigmoid = d.activation == WEKWS_HIP_ACT_SIGMOID;
  wekws::DenseParams& dp = m->dp;
  dp.head_inv_s = 1.f;
  const float* hw = blob + L.head_w().off;
  if (d.head == WEKWS_HIP_HEAD_LINEAR) {
    if (K > 16) {  // wide (CTC) heads: rows padded to a multiple of 32 so that o-tiles come in pairs (ds256_mm.hip.h)
      const int Kp = round_up(K, 32);
      std::vector<float> wp(size_t(Kp) * C, 0.f);
      std::memcpy(wp.data(), hw, size_t(K) * C * sizeof(float));
      dp.head_a16 = img.put_packed_a16(wp.data(), Kp, C, C, &dp.head_inv_s);
    } else {
      dp.head_a16 = img.put_packed_a16(hw, K, C, C, &dp.head_inv_s);
    }
    sp.head_w = img.put(hw, size_t(K) * C);
    sp.head_b = img.put(blob + L.head_b().off, K);
  } else if (d.head == WEKWS_HIP_HEAD_GLOBAL || d.head == WEKWS_HIP_HEAD_LAST) {
    const int HH = d.head_hidden;
    sp.head_w = img.put(hw, size_t(HH) * C);
    sp.head_b = img.put(blob + L.head_b().off, HH);
    sp.head_w2 = img.put(blob + L.head_w2().off, size_t(K) * HH);
    sp.head_b2 = img.put(blob + L.head_b2().off, K);
  }
  // dense-stack kernel parameters (plain TCN): same scalars, its own block table
  dp.nblocks = sched.nb; dp.idim = d.idim; dp.kpre16 = sp.kpre16; dp.ksize = ks; dp.odim = K; dp.pre_relu = d.preproc_relu;
  dp.pre_a16 = sp.pre_a16; dp.pre_b = sp.pre_b; dp.head = d.head; dp.head_hidden = d.head_hidden; dp.sigmoid = sp.sigmoid;
  dp.head_w = sp.head_w; dp.head_b = sp.head_b; dp.head_w2 = sp.head_w2; dp.head_b2 = sp.head_b2; dp.cache_len = off;
  dp.pre_inv_s = sp.pre_inv_s;
  sp.head_inv_s = dp.head_inv_s;
  // what this shape can run on: one pure function of the descriptor (route.h), shared with the CPU tests
  m->rf = wekws::conv_route_flags(d, int(wekws::ds256_stream_lds_bytes(off)), int(wekws::mdtc64_stream_lds_bytes(off)));
}

// ... and of a GRU (preprocessing, layers, classifier; the exact-f32 operands and the split-fp16 ones)
static void pack_gru(const wekws_hip_desc& d, const float* blob, Image& img, wekws_hip_model* m) {
  const int C = d.hdim, K = d.odim;
  const wekws::BlobLayout L = wekws::blob_layout(d);
  const float *wpre = blob + L.pre_w().off, *bpre = blob + L.pre_b().off, *hw = blob + L.head_w().off;
  wekws::GruParams& gp = m->gp;
  gp.pre_a = img.put_packed_a(wpre, C, d.idim, d.idim);
  gp.pre_b = img.put(bpre, C);
  gp.idim = d.idim;
  gp.kpre = round_up(d.idim, 16);
  gp.odim = K;
  gp.pre_relu = d.preproc_relu;
  gp.nlayers = d.num_layers;
  gp.sigmoid = d.activation == WEKWS_HIP_ACT_SIGMOID;
  for (int l = 0; l < d.num_layers; ++l) {
    const wekws::GruWeights lw = L.gru_layer(l);
    const float *wih = blob + lw.w_ih.off, *whh = blob + lw.w_hh.off, *bih = blob + lw.b_ih.off, *bhh = blob + lw.b_hh.off;
    gp.layer[l].a_ih = img.put_packed_a(wih, 3 * C, C, C);
    gp.layer[l].a_hh = img.put_packed_a(whh, 3 * C, C, C);
    m->gq.a_ih16[l] = img.put_packed_a16(wih, 3 * C, C, C, &m->gq.ih_inv_s[l]);
    m->gq.a_hh16[l] = img.put_packed_a16(whh, 3 * C, C, C, &m->gq.hh_inv_s[l]);
    gp.layer[l].b_ih = img.put(bih, 3 * C);
    gp.layer[l].b_hh = img.put(bhh, 3 * C);
  }
  m->gq.head_a16 = img.put_packed_a16(hw, K, C, C, &m->gq.head_inv_s);
  gp.head_w = img.put(hw, size_t(K) * C);
  gp.head_b = img.put(blob + L.head_b().off, K);
  m->gq.kpre16 = round_up(d.idim, 32);
  m->gq.pre_a16 = img.put_packed_a16(wpre, C, d.idim, d.idim, &m->gq.pre_inv_s);
  // |Wpre x + b| <= pre_alpha * max|x| + pre_beta
  l1_bound<float>(wpre, C, d.idim, d.idim, bpre, 1.00001f, &m->gq.pre_alpha, &m->gq.pre_beta);
  m->cache_len = 0;
}

// fbank of float or int16 samples
template <class S>
static int fbank_compute(wekws_hip_fbank* f, const S* pcm, int B, int nsamp, float* feats, int resident, void* stream_) {
  if (!f || !pcm || !feats) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (B < 0 || nsamp < 0) return fail(WEKWS_HIP_EINVAL, "B=%d nsamp=%d", B, nsamp);
  const int nf = wekws_hip_fbank_num_frames(f, nsamp);
  if (B == 0 || nf == 0) return WEKWS_HIP_OK;
  DeviceGuard guard(f->device);
  const int rc = wekws::launch_fbank<S>(f->fp, pcm, B, nsamp, nf, feats, resident, static_cast<hipStream_t>(stream_));
  if (rc) return fail(rc, "fbank launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}

// One forward of (B, T) on the model's device, already current: the backbone's path, then the softmax
static int forward_call(wekws_hip_model* m, const float* x, int B, int T, const float* in_cache, float* y, float* out_cache, int softmax,
                        hipStream_t stream) {
  const wekws_hip_desc& d = m->desc;
  const bool per_frame = d.head == WEKWS_HIP_HEAD_LINEAR || d.head == WEKWS_HIP_HEAD_IDENTITY;
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

// Grouped path: the rows of a bucket out of their places -- features (nb, xrow) and live planes in the forward's cache geometry
// ((outer, nb, inner): GRU (L, nb, H), every other backbone (1, nb, E)) -- and back: outputs (nb, yrow) into the rows of y, the new
// caches into the streams' other planes.
static __global__ void pool_gather_kernel(const wekws::StreamRow* __restrict__ rows, int nb, float* __restrict__ xg, int xrow,
                                          float* __restrict__ cg, int outer, int inner) {
  const wekws::StreamRow r = rows[blockIdx.x];
  const int b = blockIdx.x, step = gridDim.y * blockDim.x, e0 = blockIdx.y * blockDim.x + threadIdx.x;
  for (int e = e0; e < xrow; e += step) xg[int64_t(b) * xrow + e] = r.x[e];
  for (int e = e0; e < outer * inner; e += step) {
    const int o = e / inner, i = e - o * inner;
    cg[(int64_t(o) * nb + b) * inner + i] = r.in_cache[e];
  }
}
static __global__ void pool_scatter_kernel(const wekws::StreamRow* __restrict__ rows, int nb, const float* __restrict__ yg, int yrow,
                                           const float* __restrict__ cg, int outer, int inner) {
  const wekws::StreamRow r = rows[blockIdx.x];
  const int b = blockIdx.x, step = gridDim.y * blockDim.x, e0 = blockIdx.y * blockDim.x + threadIdx.x;
  for (int e = e0; e < yrow; e += step) r.y[e] = yg[int64_t(b) * yrow + e];
  for (int e = e0; e < outer * inner; e += step) {
    const int o = e / inner, i = e - o * inner;
    r.out_cache[e] = cg[(int64_t(o) * nb + b) * inner + i];
  }
}

static size_t pool_align(size_t v) { return (v + 255) / 256 * 256; }

// The buckets of a grouped call, one after the other on the stream: gather, the uniform forward, scatter
static int forward_streams_grouped(wekws_hip_model* m, wekws_hip_stream_cache* p, const wekws::StreamsPlan& plan,
                                   const wekws::StreamRow* d_rows, int softmax, hipStream_t stream) {
  const wekws_hip_desc& d = m->desc;
  const bool per_frame = d.head == WEKWS_HIP_HEAD_LINEAR || d.head == WEKWS_HIP_HEAD_IDENTITY;
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
    if (e != hipSuccess) { p->scratch = nullptr; return fail(e == hipErrorOutOfMemory ? WEKWS_HIP_ENOMEM : WEKWS_HIP_EDEVICE, "forward_streams: scratch of %zu bytes: %s", need, hipGetErrorString(e)); }
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
    hipLaunchKernelGGL(pool_gather_kernel, grid, dim3(256), 0, stream, rows, nb, xg, xrow, cin, p->E ? outer : 0, inner);
    if (hipGetLastError() != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "forward_streams: gather launch failed");
    if (const int rc = forward_call(m, xg, nb, n, cin, yg, cout, softmax, stream); rc != WEKWS_HIP_OK) return rc;
    hipLaunchKernelGGL(pool_scatter_kernel, grid, dim3(256), 0, stream, rows, nb, yg, yrow, cout, p->E ? outer : 0, inner);
    if (hipGetLastError() != hipSuccess) return fail(WEKWS_HIP_EDEVICE, "forward_streams: scatter launch failed");
  }
  return WEKWS_HIP_OK;
}

extern "C" {

#ifdef WEKWS_GRU_PIPE_STAMPS
// measurement build only (tools/probe/gru_stamps.py): the wall-clock stamps gru_pipe_kernel left behind
int wekws_hip_debug_gru_stamps(unsigned long long* dst, int n) {
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(wekws::gp_stamps), size_t(n) * 8) == hipSuccess ? 0 : -3;
}
#endif
const char* wekws_hip_last_error(void) { return g_err.c_str(); }
int wekws_hip_abi_version(void) { return WEKWS_HIP_ABI_VERSION; }

size_t wekws_hip_blob_elems(const wekws_hip_desc* desc) {
  if (!desc) { fail(WEKWS_HIP_EINVAL, "desc is NULL"); return 0; }
  return blob_elems(*desc);
}

int wekws_hip_create(const wekws_hip_desc* desc, const float* blob, size_t n_elems, int device,
                     wekws_hip_model** out) {
  if (!desc || !blob || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  const wekws_hip_desc& d = *desc;
  const size_t need = blob_elems(d);
  if (!need) return WEKWS_HIP_EINVAL;
  if (need != n_elems) return fail(WEKWS_HIP_EINVAL, "weight blob has %zu floats, descriptor needs %zu", n_elems, need);
  if (d.backbone == WEKWS_HIP_BACKBONE_FSMN) return create_fsmn(d, blob, n_elems, device, out);
  const float* const orig = blob;                           // (the any-shape path takes the packer's blob as it is)
  std::vector<float> balanced(blob, blob + n_elems);        // (exact power-of-two rescaling: see balance_operand_channels)
  balance_operand_channels(d, balanced.data());
  blob = balanced.data();
  // which shape the kernels run: as it is, zero-padded to the next built one, or the any-shape path -- a pure function of the
  // descriptor (route.h: conv_shape_plan / gru_shape_plan; tests/test_route.py sweeps them on the CPU)
  const wekws::ShapePlan plan = desc_conv(d) ? wekws::conv_shape_plan(d, wekws::kAmaxMaxBlocks) : wekws::gru_shape_plan(d);
  if (plan.kind == wekws::SHAPE_GENERIC) return create_generic(d, orig, n_elems, device, out);
  if (plan.kind == wekws::SHAPE_PADDED) return create_padded(d, plan, blob, device, out);
  std::optional<DeviceGuard> guard;
  wekws_hip_model* m = nullptr;
  if (const int rc = open_model(device, d, guard, &m); rc != WEKWS_HIP_OK) return rc;

  Image img;
  img.reserve(4);  // offset 0 is never a valid section
  std::vector<wekws::BlockDesc> blocks;
  std::vector<wekws::DenseBlock> dblocks;
  if (desc_conv(d)) pack_conv(d, blob, img, m, blocks, dblocks);
  else pack_gru(d, blob, img, m);
  // the promise of DEFAULT / F16X3 is fp32-level accuracy: weights outside the envelope in which the split-fp16 kernels
  // keep it (Image::spread_log2) are served by the exact-f32 kernels instead (wekws_hip_effective_precision says so)
  m->spread_log2 = img.spread_log2;
  m->rf.out_of_envelope = (d.precision == WEKWS_HIP_PRECISION_DEFAULT || d.precision == WEKWS_HIP_PRECISION_F16X3) &&
                          img.spread_log2 > WEKWS_HIP_F16X3_ENVELOPE_LOG2;
  m->ro = wekws::route_defaults(d, m->rf);
  // (measurement aid: WEKWS_GRU_NF_IN_KERNEL=0 keeps the GRU wavefront's non-finite pass a launch of its own)
  static const bool nf_in_kernel_off = [] { const char* e = std::getenv("WEKWS_GRU_NF_IN_KERNEL"); return e && e[0] == '0'; }();
  m->ro.gru_nf_in_kernel = !nf_in_kernel_off;

  if (const int rc = upload_or_destroy(m, &m->d_w, img.data.data(), img.data.size() * sizeof(float)); rc != WEKWS_HIP_OK) return rc;
  if (!blocks.empty()) {
    if (const int rc = upload_or_destroy(m, &m->d_blocks, blocks.data(), blocks.size() * sizeof(wekws::BlockDesc)); rc != WEKWS_HIP_OK) return rc;
    if (const int rc = upload_or_destroy(m, &m->d_dblocks, dblocks.data(), dblocks.size() * sizeof(wekws::DenseBlock)); rc != WEKWS_HIP_OK) return rc;
  }
  m->sp.w = m->d_w;
  m->sp.blocks = m->d_blocks;
  m->dp.w = m->d_w;
  m->dp.blocks = m->d_dblocks;
  m->gp.w = m->d_w;
  m->gq.base = m->gp;
  if (const int rc = nf_setup(m, d, orig, n_elems, WEKWS_HIP_TILE_FRAMES); rc != WEKWS_HIP_OK) {
    wekws_hip_destroy(m);
    return rc;
  }
  *out = m;
  return WEKWS_HIP_OK;
}

void wekws_hip_destroy(wekws_hip_model* m) {
  if (!m) return;
  DeviceGuard guard(m->device);
  if (m->d_w) (void)hipFree(m->d_w);
  if (m->d_blocks) (void)hipFree(m->d_blocks);
  if (m->d_dblocks) (void)hipFree(m->d_dblocks);
  nf_teardown(m);
  bool gave_up = false;
  for (auto& e : m->ws) gave_up = free_stream_buf(e) || gave_up;
  // (no return value to carry it: a failure nobody has asked about yet is at least left in wekws_hip_last_error())
  if (gave_up) {
    (void)fail(WEKWS_HIP_EDEVICE, "model destroyed with an unreported failure: a bounded wait of the GRU wavefront gave up");
    // LOUD: this is the one failure no later call can report (the last forward of a script that never asked for
    // wekws_hip_forward_status / release) -- the reference's Run would have thrown (keyword_spotting.cc:77-79)
    std::fprintf(stderr, "libwekws_hip: ERROR: %s -- the outputs of the last forward(s) on that stream are not valid\n", g_err.c_str());
  }
  delete m;
}

int wekws_hip_cache_dim(const wekws_hip_model* m) {
  if (!m) return 0;
  return m->desc.backbone == WEKWS_HIP_BACKBONE_FSMN ? m->desc.num_stack : m->user_hdim ? m->user_hdim : m->desc.hdim;
}
int wekws_hip_cache_len(const wekws_hip_model* m) { return !m ? 0 : m->user_hdim ? m->user_cache_len : m->cache_len; }

int wekws_hip_effective_precision(const wekws_hip_model* m) {
  if (!m) return fail(WEKWS_HIP_EINVAL, "NULL model");
  if (m->generic) return WEKWS_HIP_PRECISION_F32;                                     // the any-shape path: exact f32 products
  return wekws::effective_precision(m->desc, m->rf, m->ro, m->cus);              // the routes the model can take
}

float wekws_hip_weight_spread_log2(const wekws_hip_model* m) { return m ? m->spread_log2 : -1.f; }

size_t wekws_hip_cache_elems(const wekws_hip_model* m, int B) {
  if (!m || B <= 0) return 0;
  if (m->desc.backbone == WEKWS_HIP_BACKBONE_GRU) return size_t(m->desc.num_layers) * B * (m->user_hdim ? m->user_hdim : m->desc.hdim);
  if (m->desc.backbone == WEKWS_HIP_BACKBONE_FSMN) return size_t(B) * m->desc.num_stack * m->cache_len * m->desc.num_layers;
  if (m->user_hdim) return size_t(B) * m->user_hdim * m->user_cache_len;
  return size_t(B) * m->desc.hdim * m->cache_len;
}

size_t wekws_hip_output_elems(const wekws_hip_model* m, int B, int T) {
  if (!m || B <= 0 || T <= 0) return 0;
  if (m->desc.head == WEKWS_HIP_HEAD_GLOBAL || m->desc.head == WEKWS_HIP_HEAD_LAST) return size_t(B) * m->desc.odim;
  return size_t(B) * T * m->desc.odim;
}

int wekws_hip_set_option(wekws_hip_model* m, int option, int value) {
  if (!m) return fail(WEKWS_HIP_EINVAL, "NULL model");
  if (wekws::apply_route_option(m->ro, m->desc, m->rf, option, value)) return fail(WEKWS_HIP_EINVAL, "unknown option %d", option);
  return WEKWS_HIP_OK;
}

size_t wekws_hip_workspace_bytes(const wekws_hip_model* m, int B, int T) { return m ? workspace_need(m, B, T) + granule_need(m, B, T) : 0; }

// What a reservation for "calls of up to (B, T)" has to hold: the GRU's scratch is not monotonic in (B, T) (route.h:
// gru_reserve_bytes); every other path's is
static void reserve_need(const wekws_hip_model* m, int B, int T, size_t* plain, size_t* gran) {
  if (!m->generic && m->desc.backbone == WEKWS_HIP_BACKBONE_GRU)
    return wekws::gru_reserve_bytes(m->desc, m->ro, wekws::GruCall{B, T, 1, m->user_hdim != 0, m->cus}, plain, gran);
  *plain = workspace_need(m, B, T);
  *gran = 0;
}

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

int wekws_hip_release(wekws_hip_model* m, void* stream_) {
  if (!m) return fail(WEKWS_HIP_EINVAL, "NULL model");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DeviceGuard guard(m->device);
  int lkrc = WEKWS_HIP_OK;
  std::lock_guard<std::mutex> lk(m->ws_mu);
  for (size_t i = 0; i < m->ws.size(); ++i)
    if (m->ws[i].stream == stream) {
      if (m->ws[i].ptr || m->ws[i].gran || m->ws[i].ctl) (void)hipStreamSynchronize(stream);
      // an unreported failure must not vanish with the stream's buffers
      if (free_stream_buf(m->ws[i])) lkrc = fail(WEKWS_HIP_EDEVICE, "stream released with an unreported failure: a bounded wait of the GRU wavefront gave up");
      m->ws.erase(m->ws.begin() + i);
      break;
    }
  return lkrc;
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

// --------------------------------------------- the pool of stream caches, and the step over it ---------------------------------------------
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
    const int rc = fail(e == hipErrorOutOfMemory ? WEKWS_HIP_ENOMEM : WEKWS_HIP_EDEVICE, "stream_cache_create: %s", hipGetErrorString(e));
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
  const bool per_frame = d.head == WEKWS_HIP_HEAD_LINEAR || d.head == WEKWS_HIP_HEAD_IDENTITY;
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
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
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
    g_last_route = plan.conv;
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

// --------------------------------------------- fbank ---------------------------------------------
int wekws_hip_fbank_create(const wekws_hip_fbank_cfg* cfg, int device, wekws_hip_fbank** out) {
  if (!cfg || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  if (cfg->num_bins <= 0 || cfg->num_bins > wekws::kFbankMaxBins || cfg->sample_rate <= 0 || cfg->frame_length <= 0 ||
      cfg->frame_shift <= 0 || cfg->frame_length > wekws::kFbankMaxFft)
    return fail(WEKWS_HIP_EINVAL, "fbank cfg out of range");
  if (cfg->window != WEKWS_HIP_WINDOW_HAMMING && cfg->window != WEKWS_HIP_WINDOW_POVEY)
    return fail(WEKWS_HIP_EINVAL, "fbank window %d", cfg->window);
  if (cfg->frame_length <= 64)
    // (the reference would transform 64 points or fewer; frames that short -- 4 ms at 16 kHz -- have no recipe, and the
    // mel slots of a 512-point spectrum sampled every 8th bin or sparser are not laid out for it)
    return fail(WEKWS_HIP_EUNSUPPORTED, "fbank frame_length %d: frames of 65 .. 512 samples are built", cfg->frame_length);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(WEKWS_HIP_EDEVICE, "device %d of %d", device, ndev);
  DeviceGuard guard(device);
  if (!guard.ok) return fail(WEKWS_HIP_EDEVICE, "hipSetDevice(%d)", device);
  wekws_hip_fbank* f = new (std::nothrow) wekws_hip_fbank();
  if (!f) return fail(WEKWS_HIP_ENOMEM, "host allocation");
  f->device = device;
  std::vector<float> tables;
  const int empty = wekws::fbank_build_tables(cfg->num_bins, cfg->sample_rate, cfg->frame_length, cfg->frame_shift, cfg->window,
                                              &f->fp, &tables);
  if (empty >= 0) {                                           // (the reference's constructor CHECK-fails: fbank.h:81)
    delete f;
    return fail(WEKWS_HIP_EINVAL, "fbank: mel filter %d of %d covers no FFT bin (sample_rate %d, frame_length %d): fewer bins", empty,
                cfg->num_bins, cfg->sample_rate, cfg->frame_length);
  }
  hipError_t e = hipMalloc(&f->d_tables, tables.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(f->d_tables, tables.data(), tables.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (f->d_tables) (void)hipFree(f->d_tables);
    delete f;
    return fail(WEKWS_HIP_EDEVICE, "fbank table upload: %s", hipGetErrorString(e));
  }
  f->fp.tables = f->d_tables;
  f->resident_f32 = wekws::fbank_resident_groups<float>(f->fp);
  f->resident_i16 = wekws::fbank_resident_groups<int16_t>(f->fp);
  *out = f;
  return WEKWS_HIP_OK;
}

void wekws_hip_fbank_destroy(wekws_hip_fbank* f) {
  if (!f) return;
  DeviceGuard guard(f->device);
  if (f->d_tables) (void)hipFree(f->d_tables);
  delete f;
}

int wekws_hip_fbank_num_frames(const wekws_hip_fbank* f, int nsamp) {
  if (!f || nsamp < f->fp.frame_length) return 0;
  return 1 + (nsamp - f->fp.frame_length) / f->fp.frame_shift;  // fbank.h:141-142
}

int wekws_hip_fbank_compute(wekws_hip_fbank* f, const float* pcm, int B, int nsamp, float* feats, void* stream_) {
  return fbank_compute(f, pcm, B, nsamp, feats, f ? f->resident_f32 : 0, stream_);
}
int wekws_hip_fbank_compute_i16(wekws_hip_fbank* f, const int16_t* pcm, int B, int nsamp, float* feats, void* stream_) {
  return fbank_compute(f, pcm, B, nsamp, feats, f ? f->resident_i16 : 0, stream_);
}

// --------------------------------------------- context expansion + frame skip ---------------------------------------------
int wekws_hip_splice_frames(int T, int right, int skip) {
  if (skip <= 0 || right < 0 || T <= 0) return 0;
  // init_dataset.py:50  feats_ctx[:, :T - right]  -- a NEGATIVE bound (an utterance shorter than its right context) is Python's
  // "all but the last right - T": 2 T - right frames survive -- then :64-65 keeps every skip-th
  const int kept = T >= right ? T - right : (2 * T > right ? 2 * T - right : 0);
  return (kept + skip - 1) / skip;
}

int wekws_hip_splice(const float* feats, int B, int T, int F, int left, int right, int skip, float* out, void* stream_) {
  if (!feats || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (B < 0 || T < 0 || F <= 0 || left < 0 || right < 0 || skip <= 0)
    return fail(WEKWS_HIP_EINVAL, "B=%d T=%d F=%d left=%d right=%d skip=%d", B, T, F, left, right, skip);
  // init_dataset.py:45-48: the left-margin loop reads feats_ctx[:, left] -- the reference raises IndexError for left >= T (any B)
  if (left >= 1 && left >= T)
    return fail(WEKWS_HIP_EINVAL, "splice: left context %d >= T = %d (the reference's left-margin loop raises IndexError)", left, T);
  const int To = wekws_hip_splice_frames(T, right, skip);
  if (B == 0 || To == 0) return WEKWS_HIP_OK;
  if ((int64_t(B) * To * (left + right + 1) * F + 255) / 256 > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "splice: too many elements for one launch");
  const int rc = wekws::launch_splice(feats, B, T, F, left, right, skip, To, out, static_cast<hipStream_t>(stream_));
  if (rc) return fail(rc, "splice launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}

// --------------------------------------------- MFCC tail (DCT + lifter) ---------------------------------------------
int wekws_hip_dct_lifter(const float* logmel, int64_t rows, int num_bins, int num_ceps, float cepstral_lifter, float* out,
                         void* stream_) {
  if (!logmel || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (rows < 0 || num_bins <= 0 || num_bins > wekws::kMfccMaxBins || num_ceps <= 0 || num_ceps > num_bins || cepstral_lifter < 0.f)
    return fail(WEKWS_HIP_EINVAL, "rows=%lld num_bins=%d num_ceps=%d lifter=%g (need 0 < num_ceps <= num_bins <= %d)",
                (long long)rows, num_bins, num_ceps, double(cepstral_lifter), wekws::kMfccMaxBins);
  if (rows == 0) return WEKWS_HIP_OK;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return fail(WEKWS_HIP_EDEVICE, "no HIP device");
  const int rc = wekws::launch_dct_lifter(logmel, rows, num_bins, num_ceps, cepstral_lifter, out, cus, static_cast<hipStream_t>(stream_));
  if (rc) return fail(rc, "dct_lifter launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}

// --------------------------------------------- CTC first beam prune ---------------------------------------------
int wekws_hip_softmax_topk(const float* logits, int64_t rows, int K, int k, float* probs, int32_t* idx, void* stream_) {
  if (!logits || !probs || !idx) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (rows < 0 || K <= 0 || k < 1 || k > wekws::kTopkMax) return fail(WEKWS_HIP_EINVAL, "rows=%lld K=%d k=%d (k must be 1..%d)", (long long)rows, K, k, wekws::kTopkMax);
  if (rows == 0) return WEKWS_HIP_OK;
  if ((rows + 3) / 4 > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "softmax_topk: too many rows for one launch");
  const int rc = wekws::launch_softmax_topk(logits, rows, K, k, probs, idx, static_cast<hipStream_t>(stream_));
  if (rc) return fail(rc, "softmax_topk launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}

// --------------------------------------------- DET scoring ---------------------------------------------
int wekws_hip_score_maxpool(const float* scores, int B, int T, int K, const int32_t* lengths, float* max_out,
                            int32_t* argmax_out, void* stream_) {
  if (!scores || !max_out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (B < 0 || T <= 0 || K <= 0) return fail(WEKWS_HIP_EINVAL, "B=%d T=%d K=%d", B, T, K);
  if (B == 0) return WEKWS_HIP_OK;
  if ((int64_t(B) * K + 3) / 4 > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "score_maxpool: too many rows for one launch");
  const int rc = wekws::launch_det_maxpool(scores, B, T, K, lengths, max_out, argmax_out, static_cast<hipStream_t>(stream_));
  if (rc) return fail(rc, "det_maxpool launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}

static int det_false_alarms(bool text6, const float* scores, int B, int T, int K, int keyword, const int32_t* lengths,
                            const double* thresholds, int n_thr, int window_shift, int32_t* alarms, void* stream_) {
  if (!scores || !thresholds || !alarms) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (B < 0 || T <= 0 || K <= 0 || keyword < 0 || keyword >= K || n_thr <= 0 || window_shift <= 0)
    return fail(WEKWS_HIP_EINVAL, "B=%d T=%d K=%d keyword=%d n_thr=%d window_shift=%d", B, T, K, keyword, n_thr, window_shift);
  if (B == 0) return WEKWS_HIP_OK;
  if ((int64_t(B) * n_thr + 255) / 256 > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "det_false_alarms: too many items for one launch");
  const int rc = wekws::launch_det_alarms(text6, scores, B, T, K, keyword, lengths, thresholds, n_thr, window_shift, alarms,
                                          static_cast<hipStream_t>(stream_));
  if (rc) return fail(rc, "det_alarm launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}
int wekws_hip_det_false_alarms(const float* scores, int B, int T, int K, int keyword, const int32_t* lengths,
                               const double* thresholds, int n_thr, int window_shift, int32_t* alarms, void* stream_) {
  return det_false_alarms(false, scores, B, T, K, keyword, lengths, thresholds, n_thr, window_shift, alarms, stream_);
}
int wekws_hip_det_false_alarms_text(const float* scores, int B, int T, int K, int keyword, const int32_t* lengths,
                                    const double* thresholds, int n_thr, int window_shift, int32_t* alarms, void* stream_) {
  return det_false_alarms(true, scores, B, T, K, keyword, lengths, thresholds, n_thr, window_shift, alarms, stream_);
}

}  // extern "C"
