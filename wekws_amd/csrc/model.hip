// libwekws_hip.so -- C ABI (include/wekws_hip.h) over the gfx950 kernels: the model handle.  Host side only: the thread's error
// text, descriptor validation, the per-stream workspaces, destroy and the queries.  No torch, no STL types across the boundary.
// (create.hip packs and uploads the weights, forward.hip runs the forward paths, pool.hip steps many streams.)
#include <cstdio>
#include <string>

#include "gru_pipe.hip.h"
#include "model.h"

namespace {
thread_local std::string g_err;
}  // namespace

namespace wekws {
// the thread's last-error message, for every unit's fail() (host_util.h)
int set_last_error(int code, const char* msg) {
  g_err = msg;
  return code;
}
}  // namespace wekws

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

static void nf_teardown(wekws_hip_model* m) {
  if (m->nf_w) (void)hipFree(m->nf_w);
  if (m->nf_scratch) (void)hipFree(m->nf_scratch);
  if (m->nf_slots) (void)hipFree(m->nf_slots);
  if (m->nf_dev) (void)hipFree(m->nf_dev);
  m->nf_w = m->nf_scratch = nullptr;
  m->nf_slots = nullptr;
  m->nf_dev = nullptr;
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
bool free_stream_buf(StreamBuf& e) {
  if (e.ptr) (void)hipFree(e.ptr);
  if (e.gran) (void)hipFree(e.gran);
  if (e.ctl) (void)hipFree(e.ctl);
  const bool gave_up = e.err_h && *static_cast<volatile unsigned*>(e.err_h) != 0u;
  if (e.err_h) (void)hipHostFree(e.err_h);
  return gave_up;
}
// -> device pointer to at least `need` bytes owned by (model, stream); nullptr + error text on failure
char* stream_workspace(wekws_hip_model* m, hipStream_t stream, size_t need, bool granules, unsigned layout) {
  std::lock_guard<std::mutex> lk(m->ws_mu);
  StreamBuf* sb = stream_buf(m, stream);
  char*& ptr = granules ? sb->gran : sb->ptr;
  size_t& bytes = granules ? sb->gran_bytes : sb->bytes;
  if (bytes < need) {
    // Growing frees the old buffer behind a stream synchronisation -- which a stream that is being captured into a HIP
    // graph cannot do: such a call fails and names wekws_hip_reserve (no hidden synchronisation inside a capture).
    if (stream_is_capturing(stream)) {
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
      fail(hip_code(e), "workspace of %zu bytes: %s", need, hipGetErrorString(e));
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
unsigned* stream_ctl(wekws_hip_model* m, hipStream_t stream, unsigned** err_d) {
  std::lock_guard<std::mutex> lk(m->ws_mu);
  StreamBuf* sb = stream_buf(m, stream);
  if (!sb->ctl) {
    if (stream_is_capturing(stream)) {
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
int stream_health(wekws_hip_model* m, hipStream_t stream) {
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
  const bool capturing = stream_is_capturing(stream);
  if (ctl && !capturing && hipMemsetAsync(ctl + 2, 0, sizeof(unsigned), stream) == hipSuccess)
    *static_cast<volatile unsigned*>(err_h) = 0u;
  return fail(WEKWS_HIP_EDEVICE, "a bounded wait of the GRU wavefront gave up (code 0x%x: %s of stage %u): the outputs of the "
              "forwards issued on this stream since the last successful call -- including calls that returned OK while "
              "the failed launch was still queued -- are not valid", code,
              (code >> 8) == 1 ? "data" : "credit", code & 0xffu);
}

extern "C" {

const char* wekws_hip_last_error(void) { return g_err.c_str(); }
int wekws_hip_abi_version(void) { return WEKWS_HIP_ABI_VERSION; }

size_t wekws_hip_blob_elems(const wekws_hip_desc* desc) {
  if (!desc) { fail(WEKWS_HIP_EINVAL, "desc is NULL"); return 0; }
  return blob_elems(*desc);
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

}  // extern "C"
