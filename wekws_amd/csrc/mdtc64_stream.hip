// Instantiations of the MDTC h64 streaming-step kernel.  See mdtc64_stream.hip.h.
#include "mdtc64_stream.hip.h"
namespace wekws {
int launch_mdtc64_stream(const Route& r, const StackParams& P, const CallArgs& A, hipStream_t stream) {
  return with_bool(r.split, [&](auto split) {
    return launch_dyn<mdtc64_stream_kernel<split>>(r, kW16Threads, mdtc64_stream_lds_bytes(P.cache_len), 1, stream, P, A);
  });
}
}  // namespace wekws
