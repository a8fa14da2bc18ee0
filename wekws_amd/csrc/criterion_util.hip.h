// What the criterion's forward (criterion.hip.h) and backward (criterion_grad.hip.h) kernels share: limits, the small device
// helpers, and the forward CTC launch that the gradient path reuses for its loss.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wekws {

constexpr int kCritWave = 64;
constexpr int kCtcLossMaxLabels = 3000;     // LDS of the alpha kernel: (2 (2 L + 1) + L) * 4 bytes <= 64 KiB

__device__ __forceinline__ float crit_nan() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ int crit_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float crit_scale(float from, float to) { return from == -INFINITY ? 0.0f : expf(from - to); }

// lp: wekws_hip_ctc_loss's workspace; probs, stats (per frame the max and the log-sum, 2 floats): NULL or outputs
int launch_ctc_loss(const float* logits, int B, int T, int V, const int32_t* targets, int Lmax, const int32_t* logit_lengths,
                    const int32_t* target_lengths, float* loss_rows, float* loss, float* probs, float* lp, float* stats,
                    hipStream_t stream);

}  // namespace wekws
