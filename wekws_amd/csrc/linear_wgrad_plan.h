// The host plan of the Linear layers' weight and bias gradients (linear_wgrad.hip.h): the arithmetic they state, the checks
// every call makes, the slicing, the workspace, the grids and the LDS.  Pure host C++, no HIP.
//
// x (R, I) and g (R, O), float32, row-major, contiguous; grad_w (O, I) = g^T x, grad_bias (O) = the column sums of g.
//   chains   the R axis is cut into chains of kWgradChain rows counted from row 0: chain c is the rows
//            [c kWgradChain, min(R, (c + 1) kWgradChain)).  p_c[o][i] is the float32 fmaf chain fmaf(g[r][o], x[r][i], .) over
//            its rows ascending from +0 -- what v_mfma_f32_16x16x4_f32 computes from a zeroed accumulator.  The boundaries depend
//            on R alone, never on O, I or the slicing.
//   slices   a slice is a run of linear_wgrad_chains_per_slice consecutive chains (the last one may be shorter), one workgroup's
//            work for one output tile: its p_c are added in double, c ascending from +0.0, and the double partial goes to the workspace.
//   fold     grad_w[o][i] = the float32 rounding of the double sum of the slice partials, slices ascending from +0.0: rounded once.
//   bias     the same with x a column of ones: per chain the float32 sum of g[r][o], r ascending from +0, then the same doubles.
// The number of slices is a function of (R, O, I) and the constants below, never of the device, so the bits are a function of
// the inputs and the shape.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace wekws {

constexpr int kWgradChain = 512;          // rows of a float32 chain: what sets the float32 error
constexpr int kWgradTile = 64;            // a workgroup's tile of grad_w is kWgradTile (O) x kWgradTile (I); a wave owns a 32 x 32 quadrant
constexpr int kWgradThreads = 256;        // 4 waves
constexpr int kWgradStage = 32;           // rows of g and of x a stage brings to LDS; divides kWgradChain
constexpr int kWgradStride = 80;          // floats between two rows of an LDS stage: 16 mod 64, so the four k rows of an operand
                                          // read fall into four different groups of 16 banks; a multiple of 4 for the 16-byte stores
constexpr int kWgradTarget = 512;         // workgroups the partial launch aims at: two for each of the 256 CUs
constexpr int kWgradFoldThreads = 256;
constexpr int kWgradMaxDim = 65535;       // O and I

static_assert(kWgradChain % kWgradStage == 0, "a stage never straddles a chain");
static_assert(kWgradStride % 64 == 16 && kWgradStride >= kWgradTile, "the LDS row stride");

inline int64_t wgrad_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// 0 fine, else the reason the shape is refused
inline const char* linear_wgrad_shape_check(int64_t R, int64_t O, int64_t I) {
  if (R < 1) return "R must be >= 1";
  if (O < 1 || O > kWgradMaxDim) return "O must be within 1 .. 65535";
  if (I < 1 || I > kWgradMaxDim) return "I must be within 1 .. 65535";
  return nullptr;
}

// Everything below: arguments already checked by linear_wgrad_shape_check.
inline int64_t linear_wgrad_padded(int64_t n) { return wgrad_ceil_div(n, kWgradTile) * kWgradTile; }
inline int64_t linear_wgrad_tiles(int64_t O, int64_t I) { return wgrad_ceil_div(O, kWgradTile) * wgrad_ceil_div(I, kWgradTile); }
inline int64_t linear_wgrad_chains(int64_t R) { return wgrad_ceil_div(R, kWgradChain); }

// chains of a slice: enough that tiles x slices is about kWgradTarget workgroups; at least one chain
inline int64_t linear_wgrad_chains_per_slice(int64_t R, int64_t O, int64_t I) {
  const int64_t chains = linear_wgrad_chains(R);
  int64_t want = kWgradTarget / linear_wgrad_tiles(O, I);
  if (want < 1) want = 1;
  if (want > chains) want = chains;
  return wgrad_ceil_div(chains, want);
}

// 1 <= slices <= chains; the last slice may have fewer chains
inline int64_t linear_wgrad_slices(int64_t R, int64_t O, int64_t I) {
  return wgrad_ceil_div(linear_wgrad_chains(R), linear_wgrad_chains_per_slice(R, O, I));
}

// workgroups of the partial launch with grad_w wanted; without it only the bias column's tiles run (one per 64 rows of O)
inline int64_t linear_wgrad_grid(int64_t R, int64_t O, int64_t I) { return linear_wgrad_tiles(O, I) * linear_wgrad_slices(R, O, I); }
inline int64_t linear_wgrad_bias_grid(int64_t R, int64_t O, int64_t I) {
  return wgrad_ceil_div(O, kWgradTile) * linear_wgrad_slices(R, O, I);
}
inline int64_t linear_wgrad_fold_grid(int64_t O, int64_t I) { return wgrad_ceil_div(O * I + O, kWgradFoldThreads); }

// the workspace: doubles [slice][padded O][padded I], then the bias rows [slice][padded O]; bytes rounded up to 16
inline int64_t linear_wgrad_bias_offset(int64_t R, int64_t O, int64_t I) {       // in doubles
  return linear_wgrad_slices(R, O, I) * linear_wgrad_padded(O) * linear_wgrad_padded(I);
}
inline int64_t linear_wgrad_workspace_bytes(int64_t R, int64_t O, int64_t I) {
  const int64_t doubles = linear_wgrad_bias_offset(R, O, I) + linear_wgrad_slices(R, O, I) * linear_wgrad_padded(O);
  return (doubles * int64_t(sizeof(double)) + 15) / 16 * 16;
}

// static LDS of the partial kernel in bytes: two buffers of a g stage and an x stage
inline int linear_wgrad_lds_bytes() { return 2 * 2 * kWgradStage * kWgradStride * int(sizeof(float)); }

// 0 fine, else the reason the call is refused
inline const char* linear_wgrad_check(const void* x, const void* g, int64_t R, int64_t O, int64_t I, const void* grad_w,
                                      const void* grad_bias, const void* workspace, size_t workspace_bytes) {
  if (const char* why = linear_wgrad_shape_check(R, O, I)) return why;
  if (linear_wgrad_grid(R, O, I) > INT32_MAX || linear_wgrad_fold_grid(O, I) > INT32_MAX) return "grid too large for one launch";
  if (!grad_w && !grad_bias) return "neither grad_w nor grad_bias is wanted";
  if (!x || !g) return "x and g are needed";
  if (!workspace) return "the workspace is needed";
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return "the workspace must be 16-byte aligned";
  if (workspace_bytes < size_t(linear_wgrad_workspace_bytes(R, O, I))) return "the workspace is too small";
  return nullptr;
}

// linear_wgrad.hip: the partial and the fold launch for arguments already checked.  frames == 0: x (R, I) and g (R, O) row-major;
// frames > 0: x (B, I, frames) and g (B, O, frames) with R = B frames (pointwise_conv_plan.h).  0, or which launch failed.
const char* linear_wgrad_launch(const float* x, const float* g, int64_t R, int O, int I, int64_t frames, float* grad_w, float* grad_bias,
                                void* workspace, void* stream);
// The same for the K taps of a dense Conv1d (dense_conv_plan.h) in one partial and one fold launch: x (B, I, Tin), g (B, O, Tout),
// R = B Tout, tap k reads x at the frame shift k dilation - left_pad with zeros outside [0, Tin); grad_w is (O, I, K); the workspace
// is K times linear_wgrad_workspace_bytes(R, O, I).
const char* linear_wgrad_launch_taps(const float* x, const float* g, int64_t B, int64_t Tin, int64_t Tout, int O, int I, int K, int dilation,
                                     int left_pad, float* grad_w, float* grad_bias, void* workspace, void* stream);

}  // namespace wekws
