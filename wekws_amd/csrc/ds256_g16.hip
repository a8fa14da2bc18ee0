// Instantiations of the register-resident DS-TCN h256 kernel.  See ds256_g16.hip.h.
#include "ds256_g16.hip.h"
namespace wekws {
int launch_ds256_g16(const Route& r, const StackParams& P, const CallArgs& A, hipStream_t stream) {
  return with_nt(r.nt, [&](auto nt) {
    return with_bool(r.split, [&](auto split) {
      return with_bool(r.fast, [&](auto fast) {
        return with_bool(r.ctx, [&](auto ctx) {
          if constexpr (ctx && (!fast || nt < 4)) return -4;   // (no such context variant)
          else return launch_dyn<ds256_g16_kernel<nt, split, fast, ctx>>(r, kW16Threads, W16Geom<nt>::LDS_BYTES, 1, stream, P, A);
        });
      });
    });
  });
}
}  // namespace wekws
