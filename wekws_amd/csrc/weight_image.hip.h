// The host side of a model's weights: the device weight image (sections, MFMA operand packing, block-floating scales and
// bounds), the exact operand-channel balancing, and the zero-padding of a shape no kernel is built for to the next built one.
// Part of create.hip's translation unit (file-local: everything here is in the unnamed namespace); no device code.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/wekws_hip.h"
#include "blob_layout.h"
#include "route.h"

namespace {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// s = 2^(14 - floor(log2 bound)): bound * s in [2^14, 2^15); *inv = 1 / s.
// (host twin of pow2_scale in conv_stack_f16.hip.h)
inline float pow2_scale_host(float bound, float* inv) {
  uint32_t bits;
  std::memcpy(&bits, &bound, 4);
  const uint32_t e = (bits >> 23) & 0xffu;
  uint32_t se = 268u - e;
  se = se > 253u ? 253u : se;
  const uint32_t sb = se << 23, ib = (254u - se) << 23;
  float s;
  std::memcpy(&s, &sb, 4);
  std::memcpy(inv, &ib, 4);
  return s;
}

// Host-side builder of the device weight image; every section starts 16-byte aligned.
struct Image {
  std::vector<float> data;
  // Largest spread (binades) between the row maxima, or between the column maxima, of any matrix packed for the fp16
  // matrix cores.  Block floating point gives every matrix ONE power-of-two scale: an element 2^-e below the matrix
  // maximum keeps 22 - max(0, e - 16) significand bits, so a row (or a K column) whose largest element sits more than
  // ~20 binades below the matrix maximum contributes with visibly less than fp32 precision (measured through the live
  // reference: tests/golden/make_hetero_golden.py).  wekws_hip_create routes such a model to the exact-f32 kernels.
  float spread_log2 = 0.f;
  void note_spread(const float* Wsrc, int O, int Ksrc, int ld) {
    std::vector<float> rmax(size_t(O), 0.f), cmax(size_t(Ksrc), 0.f);
    float wmax = 0.f;
    for (int o = 0; o < O; ++o)
      for (int k = 0; k < Ksrc; ++k) {
        const float a = std::fabs(Wsrc[size_t(o) * ld + k]);
        if (!std::isfinite(a)) continue;
        rmax[o] = a > rmax[o] ? a : rmax[o];
        cmax[k] = a > cmax[k] ? a : cmax[k];
        wmax = a > wmax ? a : wmax;
      }
    if (!(wmax > 0.f)) return;
    auto upd = [&](const std::vector<float>& v) {
      for (float x : v)
        if (x > 0.f) {                                       // (all-zero rows / columns: padding, pruned units)
          const float sp = std::log2(wmax / x);
          spread_log2 = sp > spread_log2 ? sp : spread_log2;
        }
    };
    upd(rmax);
    upd(cmax);
  }
  uint32_t reserve(size_t n) {
    size_t off = (data.size() + 3) / 4 * 4;
    data.resize(off + n, 0.f);
    return uint32_t(off);
  }
  uint32_t put(const float* src, size_t n) {
    uint32_t off = reserve(n);
    std::memcpy(data.data() + off, src, n * sizeof(float));
    return off;
  }
  // A operand of v_mfma_f32_16x16x4_f32 for D[o][t] = sum_k W[o][k] B[k][t]:
  // element (otile, g, lane, s) = W[otile*16 + (lane&15)][g*16 + s*4 + (lane>>4)], zero beyond the source.
  uint32_t put_packed_a(const float* Wsrc, int O, int Ksrc, int ld) {
    const int Op = round_up(O, 16), Kp = round_up(Ksrc, 16);
    uint32_t off = reserve(size_t(Op) * Kp);
    float* dst = data.data() + off;
    for (int ot = 0; ot < Op / 16; ++ot)
      for (int g = 0; g < Kp / 16; ++g)
        for (int lane = 0; lane < 64; ++lane)
          for (int s = 0; s < 4; ++s) {
            const int o = ot * 16 + (lane & 15), k = g * 16 + s * 4 + (lane >> 4);
            const float v = (o < O && k < Ksrc) ? Wsrc[size_t(o) * ld + k] : 0.f;
            dst[((size_t(ot) * (Kp / 16) + g) * 64 + lane) * 4 + s] = v;
          }
    return off;
  }
  // A operand of v_mfma_f32_16x16x32_f16, operands split into fp16 hi + lo (conv_stack_f16.hip.h):
  // [o-tile][k32][hi|lo][lane][8 halves], lane l holds W[otile*16 + (l&15)][k32*32 + 8*(l>>4) + e], e = 0..7.
  // Block floating point: the matrix is stored as W * s, s the power of two that puts max|W| into [2^14, 2^15) -- the top
  // of the fp16 range, where hi + lo carries 22 bits for 16 binades below the maximum; *inv_scale = 1 / s (exact) is what
  // the kernel's epilogue multiplies the accumulator with.
  uint32_t put_packed_a16(const float* Wsrc, int O, int Ksrc, int ld, float* inv_scale) {
    const int Op = round_up(O, 16), Kp = round_up(Ksrc, 32);
    const size_t halves = size_t(Op) * Kp * 2;
    uint32_t off = reserve(halves / 2);
    _Float16* dst = reinterpret_cast<_Float16*>(data.data() + off);
    if (inv_scale) note_spread(Wsrc, O, Ksrc, ld);
    float wmax = 0.f;
    for (int o = 0; o < O; ++o)
      for (int k = 0; k < Ksrc; ++k) {
        const float a = std::fabs(Wsrc[size_t(o) * ld + k]);
        if (std::isfinite(a) && a > wmax) wmax = a;
      }
    float inv_local = 1.f;
    const float sw = inv_scale ? pow2_scale_host(wmax, inv_scale) : (void(inv_local), 1.f);   // nullptr: stored unscaled
    for (int ot = 0; ot < Op / 16; ++ot)
      for (int ks = 0; ks < Kp / 32; ++ks)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 8; ++e) {
            const int o = ot * 16 + (lane & 15), k = ks * 32 + 8 * (lane >> 4) + e;
            const float v = (o < O && k < Ksrc) ? Wsrc[size_t(o) * ld + k] * sw : 0.f;
            const _Float16 h = static_cast<_Float16>(v);
            const _Float16 l = static_cast<_Float16>(v - static_cast<float>(h));
            const size_t base = ((size_t(ot) * (Kp / 32) + ks) * 2) * 512;  // halves per (o-tile, k32, plane) = 64*8
            dst[base + lane * 8 + e] = h;
            dst[base + 512 + lane * 8 + e] = l;
          }
    return off;
  }
};

// |W a + b| <= alpha max|a| + beta for W[O][K] (leading dimension ld) and bias[O] (or none): alpha = the largest row 1-norm, summed
// in Acc, times `slack` (what the rounding of the sum and of the device's accumulation order may add), beta = max|b|.  The alphas
// feed block-floating scales: a caller's slack and Acc are part of its kernel's arithmetic.
template <class Acc>
void l1_bound(const float* W, int O, int K, int ld, const float* bias, float slack, float* alpha, float* beta) {
  float l1 = 0.f, bmax = 0.f;
  for (int o = 0; o < O; ++o) {
    Acc sum = 0;
    for (int k = 0; k < K; ++k) sum += std::fabs(Acc(W[size_t(o) * ld + k]));
    l1 = float(sum) > l1 ? float(sum) : l1;
    if (bias) bmax = std::fabs(bias[o]) > bmax ? std::fabs(bias[o]) : bmax;
  }
  *alpha = l1 * slack;
  *beta = bmax;
}

// ---------------------------------------------------------------------------------------------------------------------
// Operand-channel balancing (round 3).  A matrix product W a is unchanged when column k of W is multiplied by c_k and
// element k of a by 1 / c_k.  Where a is produced by a per-channel stage the library owns -- the depthwise conv + folded
// BN (+ ReLU) in front of a pointwise conv, the (ReLU'd) rows of the matrix in front of another matrix -- the factor moves
// into that stage's weights at no cost, exactly (c_k a power of two > 0; ReLU is positively homogeneous).  The library
// uses the freedom to give every K column of such a matrix a maximum in [1, 2): the operand tile then carries every
// channel at the magnitude of its CONTRIBUTION, one block-floating scale per matrix / tile covers the whole K axis, and the
// chained operand bounds (dw_alpha, mid_alpha, FSMN's affine bounds: products of row 1-norms) stay tight.  Without it a
// trained model that parks a 2^16 factor in a BatchNorm in front of a pointwise conv breaks the MDTC / FSMN kernels at
// 1e-3 (tests/golden/cases.py "kcol" cases, measured) although fp32 arithmetic -- the reference -- does not care.
// What must NOT be rescaled: anything the caller sees -- the residual stream (the conv caches hold it), FSMN's projections
// (its cache), GRU states.  Matrices are walked from the output side so that a matrix's rows are rescaled (by its
// consumer's balancing) before its own columns are balanced.  Exact in every precision mode: the F32 kernels compute the
// same bits as without it.
// ---------------------------------------------------------------------------------------------------------------------
// c_k for column k of W[O][K] (leading dimension ld): the power of two that puts the column maximum into [1, 2); 1 for an
// all-zero (or non-finite) column
static std::vector<float> column_balance(const float* W, int O, int K, int ld) {
  std::vector<float> c(size_t(K), 1.f);
  for (int k = 0; k < K; ++k) {
    float mx = 0.f;
    for (int o = 0; o < O; ++o) {
      const float a = std::fabs(W[size_t(o) * ld + k]);
      if (std::isfinite(a) && a > mx) mx = a;
    }
    if (mx > 0.f) {
      int e = 0;
      (void)std::frexp(mx, &e);                              // mx = f 2^e, f in [0.5, 1)  ->  mx 2^(1 - e) in [1, 2)
      e = 1 - e;
      e = e > 100 ? 100 : e < -100 ? -100 : e;
      c[k] = std::ldexp(1.f, e);
    }
  }
  return c;
}
static void scale_columns(float* W, int O, int K, int ld, const std::vector<float>& c) {
  for (int o = 0; o < O; ++o)
    for (int k = 0; k < K; ++k) W[size_t(o) * ld + k] *= c[k];
}
// rows of the producing stage: W[K][n] (n values per channel) and optionally bias[K], multiplied by 1 / c_k
static void scale_rows_inv(float* W, int K, int n, float* bias, const std::vector<float>& c) {
  for (int k = 0; k < K; ++k) {
    const float ic = 1.f / c[k];
    for (int j = 0; j < n; ++j) W[size_t(k) * n + j] *= ic;
    if (bias) bias[k] *= ic;
  }
}
static void balance_operand_channels(const wekws_hip_desc& d, float* w) {
  const int C = d.hdim, ks = d.kernel_size;
  const wekws::BlobLayout L = wekws::blob_layout(d);         // where the tensors lie: blob_layout.h
  if (d.backbone == WEKWS_HIP_BACKBONE_DS_TCN) {
    for (int i = 0; i < L.units; ++i) {
      const wekws::ConvWeights b = L.block(i);
      float* Wp = w + b.w1.off;
      const std::vector<float> c = column_balance(Wp, C, C, C);
      scale_columns(Wp, C, C, C, c);
      scale_rows_inv(w + b.wd.off, C, ks, w + b.bd.off, c);  // a_k = ReLU(dw_k(u) + b_k): c_k > 0 commutes with the ReLU
    }
  } else if (d.backbone == WEKWS_HIP_BACKBONE_MDTC) {
    for (int i = 0; i < L.units; ++i) {
      const wekws::ConvWeights b = L.block(i);
      float* W1 = w + b.w1.off; float* W2 = w + b.w2.off;
      const std::vector<float> c2 = column_balance(W2, C, C, C);
      scale_columns(W2, C, C, C, c2);
      scale_rows_inv(W1, C, C, w + b.b1.off, c2);            // mid_m = ReLU(W1[m] a + b1[m])
      const std::vector<float> c1 = column_balance(W1, C, C, C);
      scale_columns(W1, C, C, C, c1);
      scale_rows_inv(w + b.wd.off, C, ks, w + b.bd.off, c1); // a_k = BN(dw_k(u)) (linear)
    }
  } else if (d.backbone == WEKWS_HIP_BACKBONE_FSMN) {
    const int I = d.idim, A1 = d.aux[0], A2 = d.aux[1], D = d.num_stack, K = d.odim;
    float* in1 = w + L.in1_w().off; float* in2 = w + L.in2_w().off;
    float* out1 = w + L.out1_w().off; float* out2 = w + L.out2_w().off;
    // the affine of layer l, rescaled by its consumer's balancing
    auto scale_affine = [&](int l, const std::vector<float>& c) {
      const wekws::FsmnWeights lw = L.fsmn_layer(l);
      scale_rows_inv(w + lw.waff.off, C, D, w + lw.baff.off, c);
    };
    {
      const std::vector<float> c = column_balance(out2, K, A2, A2);            // out_linear2 <- out_linear1 (linear)
      scale_columns(out2, K, A2, A2, c);
      scale_rows_inv(out1, A2, C, w + L.out1_b().off, c);
    }
    {
      const std::vector<float> c = column_balance(out1, A2, C, C);             // out_linear1 <- ReLU(affine of the last layer)
      scale_columns(out1, A2, C, C, c);
      scale_affine(d.num_layers - 1, c);
    }
    for (int l = d.num_layers - 1; l >= 0; --l) {                               // Wproj(l) <- ReLU(affine(l-1)) | ReLU(in_linear2)
      float* wp = w + L.fsmn_layer(l).wproj.off;
      const std::vector<float> c = column_balance(wp, D, C, C);
      scale_columns(wp, D, C, C, c);
      if (l > 0) scale_affine(l - 1, c);
      else scale_rows_inv(in2, C, A1, w + L.in2_b().off, c);
      // (Waff(l)'s columns are fed by the memory block of Wproj(l)'s output, which is the layer's CACHE: not rescaled)
    }
    {
      const std::vector<float> c = column_balance(in2, C, A1, A1);             // in_linear2 <- in_linear1 (linear)
      scale_columns(in2, C, A1, A1, c);
      scale_rows_inv(in1, A1, I, w + L.in1_b().off, c);
    }
  }
}

// the tensors of a model's blob, in blob order (blob_layout.h)
static std::vector<wekws::BlobTensor> blob_tensors(const wekws_hip_desc& d) {
  std::vector<wekws::BlobTensor> v;
  wekws::for_each_tensor(wekws::blob_layout(d), [&](const wekws::BlobTensor& t) { v.push_back(t); });
  return v;
}

// Conv backbones whose hidden_dim C is not one of the built widths (32 / 64 / 128 / 256) run as the next built width Cp with
// the extra channels ZERO everywhere: zero rows and columns in every matrix, zero taps and biases.  A zero channel stays
// zero through the whole network (ReLU(0) = 0, residual 0 + 0) and adds exact zeros to every sum it enters, so the
// posteriors are those of the C-channel model; maxima, and with them the block-floating scales, are unchanged.  Returns the
// widened blob in the documented order (include/wekws_hip.h); `d` must be a conv descriptor that passed blob_elems().
// Likewise a kernel size ks below the built one ksp: a causal dilated conv with ks taps IS the ksp-tap conv whose first
// (oldest) ksp - ks taps are zero; only the streaming cache differs (ksp - 1 instead of ks - 1 dilations per block: the
// extra, older frames meet zero taps) -- wekws_hip_forward copies the caller's slices into / out of the tails of the wider ones.
// `built`: the descriptor of the shape it runs as (hdim Cp, kernel_size ksp).  Tensor by tensor in blob order, each into the corner of
// its built shape: rows and columns from 0, the inner axis RIGHT-aligned -- the taps of a conv are its inner axis.
static std::vector<float> pad_conv_shape(const wekws_hip_desc& d, const float* p, const wekws_hip_desc& built) {
  const std::vector<wekws::BlobTensor> from = blob_tensors(d), to = blob_tensors(built);
  std::vector<float> out(size_t(wekws::blob_layout(built).total), 0.f);
  for (size_t k = 0; k < from.size(); ++k) {
    const wekws::BlobTensor &u = from[k], &b = to[k];
    for (int64_t r = 0; r < u.rows; ++r)
      for (int c = 0; c < u.cols; ++c)
        std::memcpy(&out[size_t(b.off) + (size_t(r) * b.cols + c) * b.inner + (b.inner - u.inner)],
                    p + u.off + (size_t(r) * u.cols + c) * u.inner, u.inner * sizeof(float));
  }
  return out;
}

// GRU (torch.nn.GRU, kws_model.py:128-133) with a hidden size H below the built 128: the extra units have zero weights and
// biases in all three gates, so r = z = 1/2, n = tanh(0) = 0 and h' = (1 - z) n + z h stays 0 from a zero-padded h0 -- the
// real units never see them (zero columns).  Gate blocks [r | z | n] are padded one by one.
static std::vector<float> pad_gru_hidden(const wekws_hip_desc& d, const float* p, const wekws_hip_desc& built) {
  const int H = d.hdim, Hp = built.hdim;
  const std::vector<wekws::BlobTensor> from = blob_tensors(d), to = blob_tensors(built);
  std::vector<float> out(size_t(wekws::blob_layout(built).total), 0.f);
  for (size_t k = 0; k < from.size(); ++k) {
    const wekws::BlobTensor &u = from[k], &b = to[k];
    // rows that grow are hidden units: one block of H (preprocessing) or the three gate blocks of a layer's tensor
    const int64_t gates = b.rows == u.rows ? 1 : u.rows / H, R = u.rows / gates, Rp = b.rows == u.rows ? R : Hp;
    for (int64_t g = 0; g < gates; ++g)
      for (int64_t r = 0; r < R; ++r)
        std::memcpy(&out[size_t(b.off) + size_t(g * Rp + r) * b.cols], p + u.off + size_t(g * R + r) * u.cols, u.cols * sizeof(float));
  }
  return out;
}

}  // namespace
