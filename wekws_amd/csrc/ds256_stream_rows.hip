// Instantiations of the table-driven variant of the streaming DS-TCN h256 kernel (wekws_hip_forward_streams).  See ds256_stream.hip.h.
#include "ds256_stream.hip.h"
namespace wekws {
int launch_ds256_stream_rows(const Route& r, const StackParams& P, const CallArgs& A, hipStream_t stream) {
  if (!A.rows) return -4;
  return with_bool(r.split, [&](auto split) {
    return launch_dyn<ds256_stream_kernel<split, true>>(r, kW16Threads, ds256_stream_lds_bytes(P.cache_len), 1, stream, P, A);
  });
}
}  // namespace wekws
