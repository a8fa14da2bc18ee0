// Instantiations of the 16-wave MDTC h64 kernel.  See mdtc64_w16.hip.h.
#include "mdtc64_w16.hip.h"
namespace wekws {
int launch_mdtc64_w16(const Route& r, const StackParams& P, const CallArgs& A, hipStream_t stream) {
  return with_nt(r.nt, [&](auto nt) {
    return with_bool(r.ctx, [&](auto ctx) {
      return with_bool(r.split, [&](auto split) {
        return launch_dyn<mdtc64_w16_kernel<nt, ctx, split>>(r, kW16Threads, M16Geom<nt>::LDS_BYTES, 1, stream, P, A);
      });
    });
  });
}
}  // namespace wekws
