// Instantiations of the register-resident exact-f32 DS-TCN h256 kernel.  See ds256_g32.hip.h.
#include "ds256_g32.hip.h"
namespace wekws {
int launch_ds256_g32(const Route& r, const StackParams& P, const CallArgs& A, hipStream_t stream) {
  if (!r.fast || r.ctx) return -4;                           // (the one variant built)
  return with_nt(r.nt, [&](auto nt) {
    return launch_dyn<ds256_g32_kernel<nt>>(r, kW16Threads, W16Geom<nt>::LDS_BYTES, 1, stream, P, A);
  });
}
}  // namespace wekws
