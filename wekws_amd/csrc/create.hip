// wekws_hip_create: which shape the kernels run (route.h), the weight image (weight_image.hip.h: MFMA fragments, block-floating
// scales, every tensor from where blob_layout.h says it lies), the upload, the non-finite context.  Host side only.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <optional>

#include "model.h"
#include "ds256_stream.hip.h"
#include "mdtc64_stream.hip.h"
#include "weight_image.hip.h"

// NoSubsampling (subsampling.py:35-36) arrives as a square preprocessing matrix that is diagonal (the packer folds a CMVN into it)
static bool pre_is_diagonal(const wekws_hip_desc& d, const float* blob) {
  if (d.backbone == WEKWS_HIP_BACKBONE_FSMN || d.idim != d.hdim) return false;
  for (int r = 0; r < d.hdim; ++r)
    for (int k = 0; k < d.idim; ++k)
      if (r != k && blob[size_t(r) * d.idim + k] != 0.f) return false;
  return true;
}

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
    return fail(hip_code(e), "non-finite path setup: %s", hipGetErrorString(e));
  return WEKWS_HIP_OK;
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
  return fail(hip_code(e), "weight upload: %s", hipGetErrorString(e));
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

extern "C" int wekws_hip_create(const wekws_hip_desc* desc, const float* blob, size_t n_elems, int device,
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
