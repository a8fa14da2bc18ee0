// The host plan of the trainable GRU's recurrent scan (gru_train.hip.h): the checks every call makes, the grid, the size of
// the reserve the forward leaves for the backward and the LDS of the two kernels.  Pure host C++, no HIP.
//
// One layer, PyTorch's gate order r, z, n, H the hidden size, gi = W_ih x + b_ih computed by the caller:
//     gh = W_hh h[t-1] + b_hh      r = s(gi_r + gh_r)   z = s(gi_z + gh_z)   q = gh_n   n = tanh(gi_n + r q)
//     h[t] = (1 - z) n + z h[t-1]
// A workgroup of kGruTrainWaves waves owns kGruTrainRows batch rows for all T steps; wave w owns the hidden units
// [16 w, 16 w + 16) of all three gates, so the built hidden sizes are the multiples of 16 up to 16 kGruTrainWaves.
#pragma once
#include <stdint.h>

namespace wekws {

constexpr int kGruTrainWaves = 8;                       // waves of a workgroup; wave w owns 16 hidden units
constexpr int kGruTrainThreads = 64 * kGruTrainWaves;
constexpr int kGruTrainRows = 16;                       // batch rows a workgroup owns: the N of the 16x16x4 MFMA
constexpr int kGruTrainStride = 16;                     // floats between two units of an LDS image [unit][row]: 16 mod 32
constexpr int kGruTrainMinH = 16;
constexpr int kGruTrainMaxH = 16 * kGruTrainWaves;      // 128

// 0 fine, else the reason the shape is refused
inline const char* gru_scan_check(int64_t B, int64_t T, int64_t H) {
  if (B < 1 || T < 1) return "B and T must be >= 1";
  if (H % 16 != 0) return "H must be a multiple of 16";
  if (H < kGruTrainMinH || H > kGruTrainMaxH) return "H must be within 16 .. 128";
  if ((B + kGruTrainRows - 1) / kGruTrainRows > INT32_MAX) return "B too large for one launch";
  return nullptr;
}

// workgroups: one per tile of 16 batch rows
inline int64_t gru_scan_grid(int64_t B) { return (B + kGruTrainRows - 1) / kGruTrainRows; }

// the reserve: r, z, n, q of every (row, step) as (B, T, 4H) floats.  Arguments already checked.
inline int64_t gru_scan_reserve_bytes(int64_t B, int64_t T, int64_t H) { return B * T * 4 * H * int64_t(sizeof(float)); }

// dynamic LDS in bytes: two images of h as [H][16] (forward), two images of dgh as [3H][16] (backward)
inline int gru_scan_fwd_lds_bytes(int H) { return 2 * H * kGruTrainStride * int(sizeof(float)); }
inline int gru_scan_bwd_lds_bytes(int H) { return 2 * 3 * H * kGruTrainStride * int(sizeof(float)); }

}  // namespace wekws
