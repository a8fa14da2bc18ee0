// Instantiations of the table-driven variant of the fused FSMN kernel (wekws_hip_forward_streams).  See fsmn_f16.hip.h.
#include "fsmn_f16.hip.h"
namespace wekws {
int launch_fsmn_f16_rows(const FsmnRoute& r, const FsmnParams& P, const FsmnArgs& A, hipStream_t stream) {
  switch (r.nt * 10 + r.u) {
    case 11: return launch_fsmn_rows_nt<1, 1>(r, P, A, stream);
    case 21: return launch_fsmn_rows_nt<2, 1>(r, P, A, stream);
    case 31: return launch_fsmn_rows_nt<3, 1>(r, P, A, stream);
    case 41: return launch_fsmn_rows_nt<4, 1>(r, P, A, stream);
    case 12: return launch_fsmn_rows_nt<2, 2>(r, P, A, stream);
    case 22: return launch_fsmn_rows_nt<4, 2>(r, P, A, stream);
    case 14: return launch_fsmn_rows_nt<4, 4>(r, P, A, stream);
    default: return -4;
  }
}
}  // namespace wekws
