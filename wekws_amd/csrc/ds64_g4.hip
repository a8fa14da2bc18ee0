// Instantiations of the register-resident DS-TCN h64 kernel (one utterance per 4-wave workgroup).  See ds64_g4.hip.h.
#include "ds64_g4.hip.h"
namespace wekws {
int launch_ds64_g4(const Route& r, const StackParams& P, const CallArgs& A, hipStream_t stream) {
  if (!r.fast) return -4;                                    // (the keyword configuration only)
  return with_nt(r.nt, [&](auto nt) {
    return with_bool(r.split, [&](auto split) {
      return with_bool(A.T % nt == 0, [&](auto aligned) {
        return with_bool(r.ctx, [&](auto ctx) {
          if constexpr (ctx && nt < 4) return -4;            // (no such context variant)
          else return launch_dyn<ds64_g4_kernel<nt, split, aligned, ctx>>(r, kG4Threads, 2 * Plane<64, 16 * nt>::BYTES, 1, stream, P, A);
        });
      });
    });
  });
}
}  // namespace wekws
