// The host plan of the trainable depthwise Conv1d (depthwise_conv.hip.h): the tap table, the tiles, the fold of the tap
// gradient's partial sums, the workspace layout, the dynamic-LDS sizes and the checks every call makes.  Pure host C++, no HIP.
//
// nn.Conv1d(C, C, K, dilation=d, groups=C) over a (B, C, Tin) tensor with P zeros supplied in front of every row
// (0 <= P <= (K-1) d; Tout = Tin + P - (K-1) d; xp[n < 0] = 0):
//     y[t]  = bias + sum_k w[k] xp[t + k d - P]      k ascending
//     dx[n] = sum_k w[k] g[n + P - k d]              k ascending; terms with an index outside [0, Tout) do not exist
//     dw[k] = sum_{b,t} g[t] xp[t + k d - P]         db = sum_{b,t} g[t]
// It is fsmn_memory_plan.h's tap table in another layout: tap k is a `left` tap of index k that looks (K-1-k) d frames back from
// the last tap.  Here time is the contiguous axis, so a row is one (b, c) pair and the lanes of a wave run along t.
#pragma once
#include <stdint.h>

#include "fsmn_memory_plan.h"

namespace wekws {

constexpr int kDwConvMaxTaps = kFsmnMemMaxTaps;      // K
constexpr int kDwConvMaxWindow = kFsmnMemMaxWindow;  // (K-1) d + 1
constexpr int kDwConvThreads = 256;                  // lanes of a workgroup of every kernel
constexpr int kDwConvRows = 8;                       // (b, c) rows a workgroup owns: 32 lanes along t each
constexpr int kDwConvRowLanes = kDwConvThreads / kDwConvRows;
constexpr int kDwConvFirTile = 128;                  // output frames of a row a workgroup of the FIR kernel owns
constexpr int kDwConvGradTile = 128;                 // frames of a row a workgroup of the tap-gradient kernel sums: one partial each
constexpr int kDwConvFoldSegs = 8;                   // the fold: up to 8 segments of consecutive partials, then the segments' sums
constexpr int kDwConvFoldCols = kDwConvThreads / kDwConvFoldSegs;   // (channel, tap) pairs a workgroup of the fold owns

inline int64_t depthwise_conv_tout(int64_t Tin, int64_t K, int64_t d, int64_t P) { return Tin + P - (K - 1) * d; }
inline int64_t depthwise_conv_row_blocks(int64_t B, int64_t C) { return (B * C + kDwConvRows - 1) / kDwConvRows; }
// workgroups of the FIR kernel over rows of `L` output frames, and of the tap-gradient kernel
inline int64_t depthwise_conv_fir_tiles(int64_t B, int64_t C, int64_t L) {
  return depthwise_conv_row_blocks(B, C) * ((L + kDwConvFirTile - 1) / kDwConvFirTile);
}
inline int64_t depthwise_conv_grad_tiles(int64_t B, int64_t C, int64_t Tout) {
  return depthwise_conv_row_blocks(B, C) * ((Tout + kDwConvGradTile - 1) / kDwConvGradTile);
}
// partial sums a (channel, tap) pair has: one per batch row and frame tile
inline int64_t depthwise_conv_partials(int64_t B, int64_t Tout) { return B * ((Tout + kDwConvGradTile - 1) / kDwConvGradTile); }

// 0 fine, else the reason the shape is refused
inline const char* depthwise_conv_check(int64_t B, int64_t C, int64_t Tin, int64_t K, int64_t d, int64_t P) {
  if (B < 1 || C < 1 || Tin < 1) return "B, C and Tin must be >= 1";
  if (K < 1 || K > kDwConvMaxTaps) return "K must be in 1..32";
  if (d < 1) return "dilation must be >= 1";
  if ((K - 1) * d + 1 > kDwConvMaxWindow) return "a window above 256 frames";
  if (P < 0 || P > (K - 1) * d) return "left_pad must be in 0..(K-1)*dilation";
  if (depthwise_conv_tout(Tin, K, d, P) < 1) return "Tin + left_pad shorter than the window: no output frame";
  if (B > INT32_MAX || C > INT32_MAX || Tin > INT32_MAX) return "B, C or Tin too large for one launch";
  if (depthwise_conv_fir_tiles(B, C, Tin) > INT32_MAX) return "B * C * Tin too large for one launch";   // (Tout <= Tin)
  return nullptr;
}

// the taps in the order the products are added: k ascending; delay = frames back from the last tap
inline int depthwise_conv_taps(int K, int d, FsmnMemTap taps[kDwConvMaxTaps]) {
  for (int k = 0; k < K; ++k) taps[k] = FsmnMemTap{kFsmnMemLeft, k, (K - 1 - k) * d};
  return K;
}
inline int depthwise_conv_window(int K, int d) { return (K - 1) * d + 1; }

// the fold of `n` partials: segments of this many consecutive partials (at most kDwConvFoldSegs of them) are summed in ascending
// order, then the segments' sums in ascending segment order -- a function of the count alone (constexpr: the kernel calls it)
constexpr int64_t depthwise_conv_fold_seg_len(int64_t n) { return (n + kDwConvFoldSegs - 1) / kDwConvFoldSegs; }
// workspace: (partials, C, K + 1) doubles, the bias in column K; a multiple of 16 bytes.  Arguments already checked.
inline int64_t depthwise_conv_workspace_bytes(int64_t B, int64_t C, int64_t Tout, int64_t K) {
  return (depthwise_conv_partials(B, Tout) * C * (K + 1) * int64_t(sizeof(double)) + 15) / 16 * 16;
}
// floats of one staged row in LDS: a tile, its window and up to three frames that align its start to 16 bytes
inline int depthwise_conv_stage_stride(int tile, int window) { return (tile + window - 1 + 3 + 3) / 4 * 4; }
// dynamic LDS of the two kernels, in bytes: staged input rows, the output tile, coefficients and bias / staged x rows and g rows
inline int depthwise_conv_fir_lds_bytes(int window) {
  return kDwConvRows * (depthwise_conv_stage_stride(kDwConvFirTile, window) + kDwConvFirTile + kDwConvMaxTaps + 1) * int(sizeof(float));
}
inline int depthwise_conv_grad_lds_bytes(int window) {
  return kDwConvRows * (depthwise_conv_stage_stride(kDwConvGradTile, window) + kDwConvGradTile) * int(sizeof(float));
}

}  // namespace wekws
