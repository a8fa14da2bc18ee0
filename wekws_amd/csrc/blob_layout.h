// WHERE EVERY TENSOR OF THE WEIGHT BLOB LIES -- the executable form of the "Blob layout" comment of include/wekws_hip.h (which stays
// the document an integrator reads): blob_layout(desc) gives every tensor its offset in floats from the start of the blob and its
// shape, the size of the blob, and the tensors in blob order.  The one statement of the order on the host: wekws_hip_blob_elems, the
// packers of create.hip, the balancing and zero-padding of weight_image.hip.h and the any-shape path (generic.hip.h) read their
// pointers from here and walk nothing themselves.  Usable from device code (ROUTE_HD), but the repair routines of nonfinite.hip.h
// still walk the blob on their own: they are noinline callees of the hot kernels, and the registers a callee uses decide how its
// callers are allocated -- see the note there.
//   front   preprocessing W, b  |  FSMN: in_linear1 W, b, in_linear2 W, b
//   unit    the tensors of one residual block / GRU layer / FSMN layer; every unit of a model has the same size, so unit i lies
//           `stride` floats behind unit i - 1: block(i) / gru_layer(i) / fsmn_layer(i) are closed forms
//   back    the classifier w, b (LINEAR), w, b, w2, b2 (GLOBAL / LAST), nothing (IDENTITY)  |  FSMN: out_linear1 W, b, out_linear2 W, b
// A slot of a section is a NAME (the accessors below); blob order is slot order, and a tensor the model does not have (the depthwise
// pair of a plain TCN, the second matrix of a DS-TCN block or of a linear head) has no elements and is not enumerated.
// Plain C++ (no HIP); for descriptors that passed wekws_hip_blob_elems' validation.  tests/test_blob_layout.py holds the enumeration
// (wekws_hip_debug_blob_layout of the hooks library) and the accessors (wekws_hip_debug_blob_tensor) against the packer, wekws_amd/pack.py.
#pragma once
#include <stdint.h>

#include "../../include/wekws_hip.h"
#include "route.h"

namespace wekws {

struct BlobTensor {
  int64_t off;                    // floats from the start of the blob
  int64_t rows;                   // row-major [rows][cols][inner]: a matrix has inner = 1, a vector cols = inner = 1,
  int32_t cols, inner;            // conv taps are the inner axis ([hdim][1][ksize] depthwise, [hdim][hdim][ksize] dense)
  // (modulo 2^64, like the size_t sums of a descriptor nobody could allocate: wekws_hip_create compares the total with the blob's)
  ROUTE_HD int64_t elems() const { return int64_t(uint64_t(rows) * uint64_t(cols) * uint64_t(inner)); }
};
struct ConvWeights { BlobTensor wd, bd, w1, b1, w2, b2; };    // DS-TCN: wd, bd, w1 = Wp, b1 = bp; TCN: w1 = W[C][C][ks], b1; MDTC: all six
struct GruWeights { BlobTensor w_ih, w_hh, b_ih, b_hh; };     // gate order r, z, n within the 3 H rows
struct FsmnWeights { BlobTensor wproj, taps, waff, baff; };

struct BlobLayout {
  BlobTensor front[4], unit[6], back[4];   // unit: the tensors of unit 0
  int32_t units;
  int64_t stride, total;                   // floats of one unit; of the blob
  ROUTE_HD BlobTensor in_unit(int slot, int i) const {
    BlobTensor t = unit[slot];
    t.off += int64_t(i) * stride;
    return t;
  }
  ROUTE_HD const BlobTensor& pre_w() const { return front[0]; }
  ROUTE_HD const BlobTensor& pre_b() const { return front[1]; }
  ROUTE_HD const BlobTensor& in1_w() const { return front[0]; }
  ROUTE_HD const BlobTensor& in1_b() const { return front[1]; }
  ROUTE_HD const BlobTensor& in2_w() const { return front[2]; }
  ROUTE_HD const BlobTensor& in2_b() const { return front[3]; }
  ROUTE_HD ConvWeights block(int i) const {
    return ConvWeights{in_unit(0, i), in_unit(1, i), in_unit(2, i), in_unit(3, i), in_unit(4, i), in_unit(5, i)};
  }
  ROUTE_HD GruWeights gru_layer(int i) const { return GruWeights{in_unit(0, i), in_unit(1, i), in_unit(2, i), in_unit(3, i)}; }
  ROUTE_HD FsmnWeights fsmn_layer(int i) const { return FsmnWeights{in_unit(0, i), in_unit(1, i), in_unit(2, i), in_unit(3, i)}; }
  ROUTE_HD const BlobTensor& head_w() const { return back[0]; }
  ROUTE_HD const BlobTensor& head_b() const { return back[1]; }
  ROUTE_HD const BlobTensor& head_w2() const { return back[2]; }
  ROUTE_HD const BlobTensor& head_b2() const { return back[3]; }
  ROUTE_HD const BlobTensor& out1_w() const { return back[0]; }
  ROUTE_HD const BlobTensor& out1_b() const { return back[1]; }
  ROUTE_HD const BlobTensor& out2_w() const { return back[2]; }
  ROUTE_HD const BlobTensor& out2_b() const { return back[3]; }
};

// (the cursor of blob_layout: a tensor goes where the one before it ended)
struct BlobCursor {
  int64_t at = 0;
  ROUTE_HD void put(BlobTensor& t, int64_t rows, int cols = 1, int inner = 1) {
    t = BlobTensor{at, rows, cols, inner};
    at = int64_t(uint64_t(at) + uint64_t(t.elems()));
  }
};

ROUTE_HD inline BlobLayout blob_layout(const wekws_hip_desc& d) {
  BlobLayout L{};
  BlobCursor c;
  const int I = d.idim, C = d.hdim, K = d.odim, ks = d.kernel_size;
  const bool fsmn = d.backbone == WEKWS_HIP_BACKBONE_FSMN;
  const int A1 = d.aux[0], A2 = d.aux[1], D = d.num_stack;    // FSMN's reading of the slots (include/wekws_hip.h)
  if (fsmn) {
    c.put(L.front[0], A1, I); c.put(L.front[1], A1);          // in_linear1 (CMVN folded)
    c.put(L.front[2], C, A1); c.put(L.front[3], C);           // in_linear2
  } else {
    c.put(L.front[0], C, I); c.put(L.front[1], C);            // preprocessing
  }
  L.stride = c.at;
  L.units = d.num_layers;
  switch (d.backbone) {
    case WEKWS_HIP_BACKBONE_DS_TCN:
      c.put(L.unit[0], C, 1, ks); c.put(L.unit[1], C);        // wd, bd
      c.put(L.unit[2], C, C); c.put(L.unit[3], C);            // Wp, bp
      break;
    case WEKWS_HIP_BACKBONE_TCN:
      c.put(L.unit[2], C, C, ks); c.put(L.unit[3], C);        // W, b
      break;
    case WEKWS_HIP_BACKBONE_MDTC:
      L.units = route_blocks(d);                              // (block order: preprocessor, then stack 0 block 0 ...)
      c.put(L.unit[0], C, 1, ks); c.put(L.unit[1], C);        // wd, bd
      c.put(L.unit[2], C, C); c.put(L.unit[3], C);            // W1, b1
      c.put(L.unit[4], C, C); c.put(L.unit[5], C);            // W2, b2
      break;
    case WEKWS_HIP_BACKBONE_GRU:
      c.put(L.unit[0], 3 * int64_t(C), C); c.put(L.unit[1], 3 * int64_t(C), C);   // W_ih, W_hh
      c.put(L.unit[2], 3 * int64_t(C)); c.put(L.unit[3], 3 * int64_t(C));         // b_ih, b_hh
      break;
    default:                                                  // FSMN
      c.put(L.unit[0], D, C);                                 // Wproj (no bias)
      c.put(L.unit[1], D, 1, ks + d.stack_size);              // taps = [left, +1 on its last | right]
      c.put(L.unit[2], C, D); c.put(L.unit[3], C);            // Waff, baff
      break;
  }
  L.stride = int64_t(uint64_t(c.at) - uint64_t(L.stride));
  c.at = int64_t(uint64_t(c.at) + uint64_t(L.units - 1) * uint64_t(L.stride));
  if (fsmn) {
    c.put(L.back[0], A2, C); c.put(L.back[1], A2);            // out_linear1
    c.put(L.back[2], K, A2); c.put(L.back[3], K);             // out_linear2
  } else if (d.head == WEKWS_HIP_HEAD_LINEAR) {
    c.put(L.back[0], K, C); c.put(L.back[1], K);
  } else if (d.head == WEKWS_HIP_HEAD_GLOBAL || d.head == WEKWS_HIP_HEAD_LAST) {
    c.put(L.back[0], d.head_hidden, C); c.put(L.back[1], d.head_hidden);
    c.put(L.back[2], K, d.head_hidden); c.put(L.back[3], K);
  }
  L.total = c.at;
  return L;
}

// f(tensor) for every tensor of the blob, in blob order
template <class F>
inline void for_each_tensor(const BlobLayout& L, F f) {
  for (const BlobTensor& t : L.front)
    if (t.elems()) f(t);
  for (int i = 0; i < L.units; ++i)
    for (int s = 0; s < 6; ++s)
      if (L.unit[s].elems()) f(L.in_unit(s, i));
  for (const BlobTensor& t : L.back)
    if (t.elems()) f(t);
}

}  // namespace wekws
