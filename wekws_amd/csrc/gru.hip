// Instantiations of the three GRU kernel families (gru.hip.h, gru_f16.hip.h, gru_pipe.hip.h) and the non-finite passes that run as a
// launch of their own.  One unit: the families share device helpers whose inlining depends on who else calls them in the unit.
#include "gru_pipe.hip.h"
#include "model.h"

namespace wekws {
// runs a GRU_F32 route of select_gru_route (route.h)
int launch_gru(const GruRoute& r, const GruParams& P, const float* x, int B, int T, const float* h0, float* y, float* hn,
               hipStream_t stream) {
  if (r.family != GRU_F32 || P.kpre > 128) return -4;
  return r.nn == 4 ? launch_gru_nn<4>(r, P, x, B, T, h0, y, hn, stream)
         : r.nn == 1 ? launch_gru_nn<1>(r, P, x, B, T, h0, y, hn, stream) : -4;
}

// GRU: one workgroup per stream, behind the GRU kernels of the call (their loads sanitise, see nf_clean): a stream whose
// features or incoming states hold a NaN / Inf is re-computed; the others cost one pass over their features.
__global__ __launch_bounds__(256) void gru_nf_fix_kernel(const NfCtx* R, const float* x, int B, int T, const float* h0, float* hn,
                                                                float* y) {
  __shared__ unsigned cell;
  const int b = blockIdx.x;
  const int idim = R->d.idim, H = R->d.hdim, L = R->d.num_layers;
  bool bad = nf_scan(x + int64_t(b) * T * idim, int64_t(T) * idim, &cell);
  if (!bad && h0) bad = nf_scan_rows(h0 + int64_t(b) * H, L, H, int64_t(B) * H, &cell);
  if (bad) nf_repair_gru(R, x, int64_t(T) * idim, h0, hn, y, int64_t(T) * R->d.odim, B, T, b);
}
bool launch_gru_nf_fix(const NfCtx* nf, const float* x, int B, int T, const float* h0, float* hn, float* y, hipStream_t stream) {
  hipLaunchKernelGGL(gru_nf_fix_kernel, dim3(B), dim3(256), 0, stream, nf, x, B, T, h0, hn, y);
  return hipGetLastError() == hipSuccess;
}

// runs a GRU_F16 route of select_gru_route (route.h)
int launch_gru_f16(const GruRoute& r, const GruF16Params& Q, const GruF16Workspace& ws, const float* x, int B, int T,
                   const float* h0, float* y, float* hn, hipStream_t stream) {
  if (r.family != GRU_F16 || Q.kpre16 > 128 || Q.base.odim > 128) return -4;
  return r.nn == 2 ? launch_gru_f16_nn<2>(r, Q, ws, x, B, T, h0, y, hn, stream)
         : r.nn == 1 ? launch_gru_f16_nn<1>(r, Q, ws, x, B, T, h0, y, hn, stream) : -4;
}

// runs a GRU_PIPE route of select_gru_route (route.h); ws.nf is set exactly when the route runs the non-finite pass in the kernel
int launch_gru_pipe(const GruRoute& r, const GruF16Params& Q, const GruPipeWorkspace& ws, const float* x, int B, int T, const float* h0,
                    float* y, float* hn, hipStream_t stream) {
  if (r.family != GRU_PIPE || r.lds_bytes != kGruPipeLds || (ws.nf != nullptr) != (r.nf_in_kernel != 0) || r.stages != 2 * Q.base.nlayers ||
      r.slots < 1 || r.slots > kGruPipeMaxSlots)
    return -4;
  using G = GruF16Geom<1>;
  static DynLdsGrant grant[4];
  // <2>: at most two K steps of features in whole, 16-byte aligned octets; <4>: anything else.  pk: a time-packed first stage
  const bool k2 = r.k2, pk = r.pk;
  auto kern = k2 ? (pk ? gru_pipe_kernel<2, true> : gru_pipe_kernel<2, false>) : (pk ? gru_pipe_kernel<4, true> : gru_pipe_kernel<4, false>);
  static_assert(kGruPipeLds >= int(G::LDS_BYTES), "staging buffers");
  if (grant_dynamic_lds(kern, kGruPipeLds, grant[(k2 ? 0 : 2) + (pk ? 1 : 0)])) return -3;
  // (grid: the stage workgroups, + one non-finite workgroup per slot behind them when the route says so: gru_pipe_kernel)
  hipLaunchKernelGGL(kern, dim3(r.grid), dim3(kThreads), kGruPipeLds, stream, Q, ws, x, B, T, h0, y, hn, r.tiles, r.slots, r.slots_p, r.spw);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
}  // namespace wekws

// The same re-computation as its own launch, behind a kernel that is left exactly as it was (the register-resident kernels of
// ds64_g4.hip.h / mdtc64_g4.hip.h: one utterance per small workgroup, several workgroups per CU, at the register limit -- a
// detection branch inside them moved their register allocation into scratch).  One workgroup per utterance: a pass over its
// features (and incoming cache); what the kernel before wrote for an utterance with a NaN / Inf input is overwritten.
static __global__ __launch_bounds__(256) void conv_nf_fix_kernel(const wekws::CallArgs A, int idim, int cache_elems) {
  __shared__ unsigned cell;
  const int b = blockIdx.x;
  bool bad = wekws::nf_scan_rows(A.x + int64_t(b) * A.xs_b, A.T, idim, idim, &cell);
  if (!bad && A.in_cache) bad = wekws::nf_scan(A.in_cache + int64_t(b) * cache_elems, cache_elems, &cell);
  if (bad) wekws::nf_repair_call(A, b);
}
bool launch_conv_nf_fix(const wekws::CallArgs& a, int B, int idim, int cache_elems, hipStream_t stream) {
  hipLaunchKernelGGL(conv_nf_fix_kernel, dim3(B), dim3(256), 0, stream, a, idim, cache_elems);
  return hipGetLastError() == hipSuccess;
}

#ifdef WEKWS_GRU_PIPE_STAMPS
// measurement build only (tools/probe/gru_stamps.py): the wall-clock stamps gru_pipe_kernel left behind
extern "C" int wekws_hip_debug_gru_stamps(unsigned long long* dst, int n) {
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(wekws::gp_stamps), size_t(n) * 8) == hipSuccess ? 0 : -3;
}
#endif
