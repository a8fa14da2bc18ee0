// Instantiations of the 16-wave DS-TCN h256 kernel.  See ds256_w16.hip.h.
#include "ds256_w16.hip.h"
namespace wekws {
int launch_ds256_w16(const Route& r, const StackParams& P, const CallArgs& A, hipStream_t stream) {
  return with_nt(r.nt, [&](auto nt) {
    return with_bool(r.ctx, [&](auto ctx) {
      return with_bool(r.split, [&](auto split) {
        return launch_dyn<ds256_w16_kernel<nt, ctx, split>>(r, kW16Threads, W16Geom<nt>::LDS_BYTES, 1, stream, P, A);
      });
    });
  });
}
}  // namespace wekws
