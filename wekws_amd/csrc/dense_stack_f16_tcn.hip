// Instantiations of the dense-stack kernel (dense dilated convolutions straight from fp16 operand planes) for the plain TCN.
// See dense_stack_f16.hip.h.
#include "dense_stack_f16.hip.h"
namespace wekws {
int launch_dense_stack_f16(const Route& r, int C, const DenseParams& P, const CallArgs& A, hipStream_t stream) {
  return with_int<32, 64, 128>(C, [&](auto c) {
    return with_nt(r.nt, [&](auto nt) {
      using D = DenseGeom<KIND_TCN, c, nt>;
      return launch_dyn<dense_stack_f16_kernel<KIND_TCN, c, nt, 8>>(r, kThreads, D::LDS_BYTES, 1, stream, P, A);
    });
  });
}
}  // namespace wekws
