// The host plan of the device optimiser step (optim.hip.h): how a flat buffer of n float32 gradients is cut into tiles for the
// norm, how the tiles' partial sums are folded, how much workspace that takes, and the layout of the small state block the
// three kernels hand to each other.  Pure host C++, no HIP.
//
// The n floats are cut into tiles of kOptimTileFloats consecutive floats, one workgroup a tile; a tile leaves one double in the
// workspace.  Up to kOptimFoldSeg partials are folded by one workgroup in one fixed order; more are folded in two stages
// (segments of kOptimFoldSeg tiles, then the segments' sums).  Tile size and fold order are constants: the order in which the
// squares are added is a function of n alone, never of the device's CU count.
#pragma once
#include <stdint.h>

namespace wekws {

constexpr int kOptimThreads = 256;                     // lanes of a workgroup of every kernel
constexpr int kOptimTileFloats = 4096;                 // floats a tile of the norm reads: four 16-byte loads a lane
constexpr int kOptimFoldSeg = 256;                     // partials one workgroup folds: one a lane
constexpr int64_t kOptimMaxElems = int64_t(kOptimFoldSeg) * kOptimFoldSeg * kOptimTileFloats;   // 2^28: what two stages fold

// The state block: device memory the caller owns and zeroes before the first step.  clip_fold_kernel writes all of it but
// the two counters, which it advances; adam_apply_kernel only reads it.
struct OptimState {
  int64_t step;        //  0  steps applied so far (after the fold: the step under way included)
  int64_t skipped;     //  8  steps not applied because the norm was not finite
  double norm;         // 16  the gradient's 2-norm of the last call, from the double sum
  double bc1;          // 24  1 - beta1^step
  double bc2sqrt;      // 32  sqrt(1 - beta2^step)
  float coef;          // 40  min(1, max_norm / (norm + 1e-6)) of the last call; 1 without clipping
  float norm_f32;      // 44  float32(norm): what clip_grad_norm_ returns
  int32_t apply;       // 48  1: the last call stepped; 0: it left params and moments as they were
  int32_t finite;      // 52  isfinite(norm_f32)
  float step_size;     // 56  float32(lr / bc1) of the step under way
  float bc2sqrt_f32;   // 60  float32(bc2sqrt)
};
static_assert(sizeof(OptimState) == 64, "the state block is 64 bytes (include/wekws_hip.h documents the offsets)");

// 0 fine, 1 refused: n outside 1 .. kOptimMaxElems
inline int optim_check(int64_t n) { return n < 1 || n > kOptimMaxElems; }
inline int64_t optim_tiles(int64_t n) { return (n + kOptimTileFloats - 1) / kOptimTileFloats; }
// more than kOptimFoldSeg tiles are folded in two stages: segments of kOptimFoldSeg tiles first, then the segments' sums
inline int64_t optim_fold_segments(int64_t tiles) { return tiles > kOptimFoldSeg ? (tiles + kOptimFoldSeg - 1) / kOptimFoldSeg : 0; }
// workspace: one double a tile, then one a segment; a multiple of 16 bytes
inline int64_t optim_workspace_bytes(int64_t n) {
  const int64_t tiles = optim_tiles(n);
  return ((tiles + optim_fold_segments(tiles)) * int64_t(sizeof(double)) + 15) / 16 * 16;
}

}  // namespace wekws
