// Instantiations of the streaming (LDS-resident cache) 16-wave DS-TCN h256 kernel.  See ds256_stream.hip.h.
#include "ds256_stream.hip.h"
namespace wekws {
int launch_ds256_stream(const Route& r, const StackParams& P, const CallArgs& A, hipStream_t stream) {
  return with_bool(r.split, [&](auto split) {
    return launch_dyn<ds256_stream_kernel<split>>(r, kW16Threads, ds256_stream_lds_bytes(P.cache_len), 1, stream, P, A);
  });
}
}  // namespace wekws
