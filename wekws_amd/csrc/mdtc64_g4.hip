// Instantiations of the register-resident MDTC kernels (one utterance per workgroup of C / 16 waves).  See mdtc64_g4.hip.h.
#include "mdtc64_g4.hip.h"
namespace wekws {
int launch_mdtc_g4(const Route& r, int C, const StackParams& P, const CallArgs& A, hipStream_t stream) {
  if (!r.fast) return -4;                                    // (keyword or pooled heads only)
  const bool pooled = P.head == HEAD_GLOBAL || P.head == HEAD_LAST;
  return with_int<32, 64>(C, [&](auto c) {
    return with_nt(r.nt, [&](auto nt) {
      return with_bool(r.split, [&](auto split) {
        return with_bool(pooled, [&](auto pool) {
          return with_bool(A.T % nt == 0, [&](auto aligned) {
            return with_bool(r.ctx, [&](auto ctx) {
              // (no such variant: a context variant for pooled heads or < 4 tiles; an unaligned tail of one tile)
              if constexpr ((ctx && (pool || nt < 4)) || (nt == 1 && !aligned)) return -4;
              else return launch_dyn<mdtc_g4_kernel<c, nt, split, pool, aligned, ctx>>(r, c * 4, 2 * Plane<c, 16 * nt>::BYTES, 1, stream, P, A);
            });
          });
        });
      });
    });
  });
}
}  // namespace wekws
