// The host plan of the global CMVN statistics (tools/compute_cmvn_stats.py:26-72, 128-151 of the reference): how a call over
// (B, T, D) features is cut into tiles, and how much scratch the tiles' partial sums take.  Pure host C++, no HIP.
//
// The B * T frames of a call are numbered row by row (frame f = b * T + t) and cut into tiles of F consecutive frames, one
// workgroup a tile.  F follows from D alone -- a tile is about kCmvnTileFloats features wherever D allows it -- so the order
// in which a call's features are added is a function of (B, T, D): never of the device's CU count, never of `lengths`.
// Every tile leaves 2 D doubles in scratch (the sums, then the sums of squares); they are folded in one fixed order: up to 64
// tiles by one launch, more in two stages (segments of 64 tiles, then the segments), which is again a function of the shape.
#pragma once
#include <stdint.h>

namespace wekws {

constexpr int kCmvnMaxDim = 4096;            // D of a handle: 1 .. 4096
constexpr int kCmvnThreads = 256;            // lanes of a workgroup of either kernel
constexpr int kCmvnTileFloats = 8192;        // features a tile reads, D permitting
constexpr int kCmvnFoldCols = 16;            // bins a workgroup of the fold owns ...
constexpr int kCmvnFoldLanes = kCmvnThreads / kCmvnFoldCols;   // ... with this many lanes a bin, tile i on lane i mod 16
constexpr int kCmvnFoldSeg = 64;             // tiles a workgroup of the fold's first stage takes

// a call's shape: 0 fine, 1 refused (D outside 1..4096, B or T negative, or more than 2^31 - 1 frames)
inline int cmvn_stats_check(int64_t B, int64_t T, int64_t D) {
  if (D < 1 || D > kCmvnMaxDim || B < 0 || T < 0) return 1;
  if (T > 0 && B > 0x7fffffffLL / T) return 1;
  return 0;
}

inline int64_t cmvn_tile_frames(int64_t D) { return kCmvnTileFloats / D > 1 ? kCmvnTileFloats / D : 1; }
inline int64_t cmvn_tiles(int64_t B, int64_t T, int64_t D) { return (B * T + cmvn_tile_frames(D) - 1) / cmvn_tile_frames(D); }
// more than kCmvnFoldSeg tiles are folded in two stages: segments of kCmvnFoldSeg tiles first, then the segments' sums
inline int64_t cmvn_fold_segments(int64_t tiles) { return tiles > kCmvnFoldSeg ? (tiles + kCmvnFoldSeg - 1) / kCmvnFoldSeg : 0; }
// scratch: the tiles' partials, then the segments'
inline int64_t cmvn_scratch_bytes(int64_t B, int64_t T, int64_t D) {
  const int64_t tiles = cmvn_tiles(B, T, D);
  return (tiles + cmvn_fold_segments(tiles)) * 2 * D * int64_t(sizeof(double));
}

// Frame f lies in row f / T.  The kernel divides by multiplying: for 0 <= n < 2^31 and 1 <= d < 2^31,
//   n / d == (uint64(n) * mul) >> shift   with L = ceil(log2 d), shift = 31 + L, mul = ceil(2^shift / d) <= 2^32 - 1
// (Granlund & Montgomery, Division by Invariant Integers using Multiplication, 1994: mul d - 2^shift = e with 0 <= e < d <= 2^L,
// and the quotient is exact while n e < 2^shift, which n < 2^31 and e < 2^L give.)
struct CmvnDiv {
  uint32_t mul;
  int shift;
};
inline CmvnDiv cmvn_div(int64_t d) {
  int L = 0;
  while ((int64_t(1) << L) < d) ++L;
  const uint64_t p = uint64_t(1) << (31 + L);
  return CmvnDiv{uint32_t((p + uint64_t(d) - 1) / uint64_t(d)), 31 + L};
}

// Inside a tile: bins across the lanes, and where D leaves room (D <= 128) several frames side by side.
//   W = min(D, 256) bins a pass, G = 256 / W frames side by side; lane = g * W + c reads frames g, g + G, ... of bin c
//   (consecutive lanes, consecutive addresses: G whole frames are one contiguous run); D > 256 takes ceil(D / 256) passes.
inline int cmvn_lane_bins(int D) { return D < kCmvnThreads ? D : kCmvnThreads; }
inline int cmvn_lane_frames(int D) { return kCmvnThreads / cmvn_lane_bins(D); }

}  // namespace wekws
