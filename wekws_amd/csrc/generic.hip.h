// ANY-SHAPE path (round 5): every backbone / head / size the reference's init_model accepts (wekws/model/kws_model.py:97-214 takes
// any hidden_dim, kernel_size, num_layers ...) that the specialised kernels of this directory are NOT built for -- conv
// backbones wider than 256 channels (MDTC: 128), kernel sizes above 8 / 5, more residual blocks than the block-floating
// kernels track, GRU hidden sizes above 128 / more than 4 layers / pooled heads, FSMN layers that do not fit the LDS tile or
// whose weights fall outside the split-fp16 envelope -- and an FSMN for which precision F32 is requested.  Before round 5 those
// were WEKWS_HIP_EUNSUPPORTED (the reference runs them), resp. served with different rounding.
//
// One small family instead of one kernel per shape: activations live in HBM as (B, T, C) rows, every layer is a launch,
// all arithmetic is exact f32 (v_mfma_f32_16x16x4_f32 / v_fma_f32: every product exact, f32 accumulation, like the reference's fp32 math):
//   gen_gemm_kernel   Y = epilogue(X W^T + b): Linear / 1x1 conv / one tap of a dense conv; 64 x 64 tiles through LDS, f32 MFMA
//   gen_ctx_kernel    [cache | h] of a block as one (B, pad + T, C) buffer (tcn.py:45-53, mdtc.py:98-104, fsmn.py:228-236) and,
//                     from the same pass, the block's slice of the returned cache (its last `pad` rows)
//   gen_dw_kernel     depthwise dilated conv over that buffer (tcn.py:102-109, mdtc.py:55-58; the FSMN memory block
//                     fsmn.py:214-253 is the same sum with left_order + right_order taps and the identity folded into one of them)
//   gen_gru_cell_kernel   torch.nn.GRU's cell (gate order r, z, n) on gi = W_ih x + b_ih (all steps at once) and gh = W_hh h + b_hh
//   gen_mean_kernel / gen_last_kernel / gen_add_kernel    GlobalClassifier's mean (classifier.py:27), LastClassifier's row
//                     (classifier.py:39), MDTC's sum of stack outputs (mdtc.py:270-273)
// It is a correctness path, not a roofline one (20 .. 40 TFLOP/s: DS-TCN with 512 channels 162 k utt/s at B = 1024 x 98 frames):
// the recipes the reference ships all run on the specialised kernels.
// The weight blob is the host packer's (include/wekws_hip.h: BatchNorm and CMVN folded), uploaded as it is.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/wekws_hip.h"
#include "blob_layout.h"
#include "conv_stack.hip.h"

namespace wekws {

struct GenericModel {
  bool pre_diag = false;         // the preprocessing matrix is diagonal (NoSubsampling)
  wekws_hip_desc d{};
  const float* w = nullptr;      // the packer's blob on the device
  int cache_len = 0;             // conv: sum of paddings; fsmn: left_order - 1 + right_order; gru: 0
};

inline int gen_cache_len(const wekws_hip_desc& d) {
  if (d.backbone == WEKWS_HIP_BACKBONE_GRU) return 0;
  if (d.backbone == WEKWS_HIP_BACKBONE_FSMN) return d.kernel_size - 1 + d.stack_size;
  return int(conv_schedule(d).cache_len);                    // route.h
}
// widest row any intermediate of the model has (floats)
inline int gen_width(const wekws_hip_desc& d) {
  int w = std::max(d.hdim, d.odim);
  w = std::max(w, d.head_hidden);
  if (d.backbone == WEKWS_HIP_BACKBONE_GRU) w = std::max(w, 3 * d.hdim);
  if (d.backbone == WEKWS_HIP_BACKBONE_FSMN) w = std::max(std::max(w, d.num_stack), std::max(d.aux[0], d.aux[1]));
  return w;
}
inline size_t gen_al(size_t v) { return (v + 255) / 256 * 256; }
// scratch of one forward: four (B T, width) matrices, the [cache | h] buffer, GRU step buffers
inline size_t gen_workspace_bytes(const GenericModel& m, int B, int T) {
  const wekws_hip_desc& d = m.d;
  const size_t rows = size_t(B) * T, w = gen_width(d);
  int pmax = 0;
  if (d.backbone == WEKWS_HIP_BACKBONE_FSMN) pmax = m.cache_len;
  else if (d.backbone != WEKWS_HIP_BACKBONE_GRU)
    pmax = conv_schedule(d).max_pad;
  const size_t cu = d.backbone == WEKWS_HIP_BACKBONE_FSMN ? d.num_stack : d.hdim;
  size_t n = 4 * gen_al(rows * w * 4) + gen_al(size_t(B) * (pmax + T) * cu * 4);
  if (d.backbone == WEKWS_HIP_BACKBONE_GRU) n += gen_al(size_t(B) * 3 * d.hdim * 4) + gen_al(size_t(B) * d.hdim * 4);
  return n;
}

// The forward of wekws_hip_forward for a GenericModel (everything but the trailing softmax, which the caller applies).
// ws: gen_workspace_bytes(m, B, T) bytes of scratch.  Returns 0, or -3 if a launch failed.
// Defined in generic.hip with the gen_* kernels, the one unit that emits them.
int generic_forward(const GenericModel& m, const float* x, int B, int T, const float* in_cache, float* y, float* out_cache,
                    char* ws, hipStream_t st, hipError_t* launch_error = nullptr);

}  // namespace wekws
