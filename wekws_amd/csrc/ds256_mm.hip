// Instantiations of the all-matrix-core DS-TCN h256 kernel.  See ds256_mm.hip.h.
#include "ds256_mm.hip.h"
namespace wekws {
int launch_ds256_mm(const Route& r, const StackParams& P, uint32_t head_a16, const CallArgs& A, hipStream_t stream) {
  const int gy = A.head_slices > 1 ? A.head_slices : 1;
  return with_nt(r.nt, [&](auto nt) {
    return with_bool(r.ctx, [&](auto ctx) {
      return launch_dyn<ds256_mm_kernel<nt, ctx>>(r, kW16Threads, MmGeom<nt>::LDS_BYTES, gy, stream, P, A, head_a16);
    });
  });
}
}  // namespace wekws
