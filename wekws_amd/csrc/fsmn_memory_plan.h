// The host plan of the trainable FSMN memory block (fsmn_memory.hip.h): the tap table, the frame tiles, the fold of the tap
// gradient's partial sums, the workspace layout and the checks every call makes.  Pure host C++, no HIP.
//
// The block is a causal sparse FIR per channel.  With R = rorder * rstride and x[n < 0] = 0,
//     y[t] = sum_k c_k x[t - d_k]        over the 1 + lorder + rorder taps below, in this order
//     dx[n] = sum_k c_k g[n + d_k]       the same taps with the delays negated (terms with n + d_k >= T do not exist)
//     dc_k  = sum_{b,t} g[t] x[t - d_k]  for the lorder + rorder taps that have a weight
// The table says where a tap's coefficient comes from and how many frames it looks back; it says nothing about how the
// tensor lies in memory, so a (B, C, T) depthwise convolution is planned by the same table (depthwise_conv_plan.h).
#pragma once
#include <stdint.h>

namespace wekws {

constexpr int kFsmnMemMaxTaps = 32;          // lorder + rorder (route.h's kFsmnMaxTaps: what the packed model serves)
constexpr int kFsmnMemMaxWindow = 256;       // frames a tile looks back, the current one included: the largest delay + 1
constexpr int kFsmnMemThreads = 256;         // lanes of a workgroup of every kernel
constexpr int kFsmnMemChannels = 32;         // channels a workgroup owns: one 128-byte line of every frame
constexpr int kFsmnMemFirTile = 64;          // output frames a workgroup of the FIR kernel owns
constexpr int kFsmnMemGradTile = 128;        // frames a workgroup of the tap-gradient kernel sums: one partial a tile
constexpr int kFsmnMemFoldSegs = 8;          // the fold: up to 8 segments of consecutive tiles, then the segments' sums

enum FsmnMemSource { kFsmnMemSkip = 0, kFsmnMemLeft = 1, kFsmnMemRight = 2 };

struct FsmnMemTap {
  int source;   // kFsmnMemSkip: the coefficient is 1;  Left / Right: w_left[d, index] / w_right[d, index]
  int index;
  int delay;    // frames back, >= 0
};

// (row, frame tile) pairs: the first grid dimension of the FIR kernel and of the tap-gradient kernel
inline int64_t fsmn_memory_fir_tiles(int64_t B, int64_t T) { return B * ((T + kFsmnMemFirTile - 1) / kFsmnMemFirTile); }
inline int64_t fsmn_memory_grad_tiles(int64_t B, int64_t T) { return B * ((T + kFsmnMemGradTile - 1) / kFsmnMemGradTile); }

// 0 fine, else the reason the shape is refused
inline const char* fsmn_memory_check(int64_t B, int64_t T, int64_t D, int64_t lorder, int64_t lstride, int64_t rorder, int64_t rstride) {
  if (B < 1 || T < 1 || D < 1) return "B, T and D must be >= 1";
  if (lorder < 1 || rorder < 1) return "lorder and rorder must be >= 1";
  if (lstride < 1 || rstride < 1) return "lstride and rstride must be >= 1";
  if (lorder + rorder > kFsmnMemMaxTaps) return "lorder + rorder above 32 taps";
  if (rorder * rstride + (lorder - 1) * lstride + 1 > kFsmnMemMaxWindow) return "a window above 256 frames";
  if (B > INT32_MAX || T > INT32_MAX || D > int64_t(65535) * kFsmnMemChannels) return "B, T or D too large for one launch";
  if (fsmn_memory_fir_tiles(B, T) > INT32_MAX) return "B * T too large for one launch";
  return nullptr;
}

// the taps in the order the products are added: skip term, left taps with i ascending, right taps with j ascending
inline int fsmn_memory_taps(int lorder, int lstride, int rorder, int rstride, FsmnMemTap taps[1 + kFsmnMemMaxTaps]) {
  const int R = rorder * rstride;
  int n = 0;
  taps[n++] = FsmnMemTap{kFsmnMemSkip, 0, R};
  for (int i = 0; i < lorder; ++i) taps[n++] = FsmnMemTap{kFsmnMemLeft, i, R + (lorder - 1 - i) * lstride};
  for (int j = 0; j < rorder; ++j) taps[n++] = FsmnMemTap{kFsmnMemRight, j, R - (j + 1) * rstride};
  return n;
}
inline int fsmn_memory_window(int lorder, int lstride, int rorder, int rstride) {
  return rorder * rstride + (lorder - 1) * lstride + 1;
}

// the fold of `tiles` partials: segments of this many consecutive tiles (at most kFsmnMemFoldSegs of them) are summed in
// ascending tile order, then the segments' sums in ascending segment order -- a function of the tile count alone
// (constexpr: the fold kernel calls it too)
constexpr int64_t fsmn_memory_fold_seg_len(int64_t tiles) { return (tiles + kFsmnMemFoldSegs - 1) / kFsmnMemFoldSegs; }
// workspace: (tiles, lorder + rorder, D) doubles; a multiple of 16 bytes.  Arguments already checked.
inline int64_t fsmn_memory_workspace_bytes(int64_t B, int64_t T, int64_t D, int64_t lorder, int64_t rorder) {
  return (fsmn_memory_grad_tiles(B, T) * (lorder + rorder) * D * int64_t(sizeof(double)) + 15) / 16 * 16;
}
// dynamic LDS of the two kernels, in bytes: rows of kFsmnMemChannels floats
inline int fsmn_memory_fir_lds_bytes(int window, int ntaps) {
  return (kFsmnMemFirTile + window - 1 + ntaps) * kFsmnMemChannels * int(sizeof(float));
}
inline int fsmn_memory_grad_lds_bytes(int window) {
  return (2 * kFsmnMemGradTile + window - 1) * kFsmnMemChannels * int(sizeof(float));
}

}  // namespace wekws
