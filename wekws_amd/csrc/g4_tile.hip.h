// What the register-resident kernels with ONE utterance per workgroup of C / 16 waves share (mdtc_g4_kernel: MDTC h64 / h32,
// mdtc64_g4.hip.h; ds64_g4_kernel: DS-TCN h64, ds64_g4.hip.h) on top of the lane-major register tile of lane_tile.hip.h: the
// thread count, the feature items they stage (ds256_w16.hip.h, by name) and two one-line helpers.  The phases the two kernels
// have in common (geometry, features, preprocessing, context load, hand-over, keyword head, tail) are written out in both:
// behind a call boundary none of them compiles to the same instructions, and both kernels sit at the 128-register limit of
// four workgroups per CU ("The lane-major register tile, once").
#pragma once
#include "ds256_w16.hip.h"                                   // the feature items: W16XItem, w16_fetch_x, w16_x_amax_bits, w16_put_x
#include "lane_tile.hip.h"

namespace wekws {

constexpr int kG4Threads = 256;

// (wave-uniform values, moved to scalar registers: the kernels are at the 128-register limit)
__device__ __forceinline__ float g4_uni(float v) {
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}
// the maximum that bounds a block's depthwise rows: its input tile's and (CTX) the incoming cache's
template <bool CTX>
__device__ __forceinline__ float g4_input_amax(const AmaxCell* amax_cells, int bi) {
  return CTX ? fmaxf(amax_read(amax_cells + 2 + bi), amax_read(amax_cells + 1)) : amax_read(amax_cells + 2 + bi);
}

}  // namespace wekws
