// The trainable FSMN memory block: launches and C entry points (kernels: fsmn_memory.hip.h; the plan: fsmn_memory_plan.h).
#include "fsmn_memory.hip.h"

#include "host_util.h"

namespace {

using wekws::FsmnMemArgs;

// the shape and the tap table as the kernels read them; sign +1: rows are frames t0 - halo ... and a tap reads halo - delay
// rows on (forward, tap gradient); -1: rows are frames t0 ... and a tap reads delay rows on (the input gradient)
FsmnMemArgs make_args(int T, int D, int lorder, int lstride, int rorder, int rstride, int sign, int tile) {
  wekws::FsmnMemTap taps[1 + wekws::kFsmnMemMaxTaps];
  FsmnMemArgs a{};
  a.T = T;
  a.D = D;
  a.lorder = lorder;
  a.rorder = rorder;
  a.ntaps = wekws::fsmn_memory_taps(lorder, lstride, rorder, rstride, taps);
  a.halo = wekws::fsmn_memory_window(lorder, lstride, rorder, rstride) - 1;
  a.tiles_t = (T + tile - 1) / tile;
  for (int k = 0; k < a.ntaps; ++k) {
    a.off[k] = int16_t(sign > 0 ? a.halo - taps[k].delay : taps[k].delay);
    a.source[k] = uint8_t(taps[k].source);
    a.index[k] = uint8_t(taps[k].index);
  }
  return a;
}

// 16-byte accesses where every row of every tensor starts on a 16-byte boundary
bool can_vec(int D, const void* p, const void* q) { return D % 4 == 0 && aligned16(p) && aligned16(q); }

template <bool BWD>
int launch_fir(const float* in, float* out, int B, const float* wl, const float* wr, const FsmnMemArgs& a, hipStream_t s) {
  const dim3 grid(unsigned(wekws::fsmn_memory_fir_tiles(B, a.T)), unsigned((a.D + wekws::kFsmnMemChannels - 1) / wekws::kFsmnMemChannels));
  const size_t lds = size_t(wekws::fsmn_memory_fir_lds_bytes(a.halo + 1, a.ntaps));
  if (can_vec(a.D, in, out))
    hipLaunchKernelGGL((wekws::fsmn_memory_fir_kernel<4, BWD>), grid, dim3(wekws::kFsmnMemThreads), lds, s, in, out, wl, wr, a);
  else
    hipLaunchKernelGGL((wekws::fsmn_memory_fir_kernel<1, BWD>), grid, dim3(wekws::kFsmnMemThreads), lds, s, in, out, wl, wr, a);
  return hipGetLastError() != hipSuccess;
}

int check_shape(const char* what, int B, int T, int D, int lorder, int lstride, int rorder, int rstride) {
  if (const char* why = wekws::fsmn_memory_check(B, T, D, lorder, lstride, rorder, rstride))
    return fail(WEKWS_HIP_EINVAL, "%s: %s (B=%d T=%d D=%d lorder=%d lstride=%d rorder=%d rstride=%d)", what, why, B, T, D, lorder, lstride,
                rorder, rstride);
  return WEKWS_HIP_OK;
}

}  // namespace

extern "C" {

size_t wekws_hip_fsmn_memory_workspace_bytes(int B, int T, int D, int lorder, int rorder) {
  if (wekws::fsmn_memory_check(B, T, D, lorder, 1, rorder, 1)) {    // (strides do not enter the size; the calls check the window)
    fail(WEKWS_HIP_EINVAL, "fsmn_memory_workspace_bytes: B=%d T=%d D=%d lorder=%d rorder=%d", B, T, D, lorder, rorder);
    return 0;
  }
  return size_t(wekws::fsmn_memory_workspace_bytes(B, T, D, lorder, rorder));
}

int wekws_hip_fsmn_memory_forward(const float* x, int B, int T, int D, const float* w_left, int lorder, int lstride, const float* w_right,
                                  int rorder, int rstride, float* y, void* stream) {
  if (!x || !w_left || !w_right || !y) return fail(WEKWS_HIP_EINVAL, "fsmn_memory_forward: NULL argument");
  if (const int rc = check_shape("fsmn_memory_forward", B, T, D, lorder, lstride, rorder, rstride)) return rc;
  const FsmnMemArgs a = make_args(T, D, lorder, lstride, rorder, rstride, +1, wekws::kFsmnMemFirTile);
  if (launch_fir<false>(x, y, B, w_left, w_right, a, static_cast<hipStream_t>(stream)))
    return fail(WEKWS_HIP_EDEVICE, "fsmn_memory_forward launch failed");
  return WEKWS_HIP_OK;
}

int wekws_hip_fsmn_memory_backward(const float* x, const float* grad_y, int B, int T, int D, const float* w_left, int lorder, int lstride,
                                   const float* w_right, int rorder, int rstride, float* grad_x, float* grad_w_left, float* grad_w_right,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !grad_y || !w_left || !w_right) return fail(WEKWS_HIP_EINVAL, "fsmn_memory_backward: NULL argument");
  if (const int rc = check_shape("fsmn_memory_backward", B, T, D, lorder, lstride, rorder, rstride)) return rc;
  if ((grad_w_left == nullptr) != (grad_w_right == nullptr))
    return fail(WEKWS_HIP_EINVAL, "fsmn_memory_backward: grad_w_left and grad_w_right are wanted together or not at all");
  if (grad_w_left)                                                  // the tap gradient's partial sums
    if (const int rc = check_workspace("fsmn_memory_backward", workspace, workspace_bytes,
                                       size_t(wekws::fsmn_memory_workspace_bytes(B, T, D, lorder, rorder)),
                                       "wekws_hip_fsmn_memory_workspace_bytes"))
      return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  bool bad = false;
  if (grad_x) {
    const FsmnMemArgs a = make_args(T, D, lorder, lstride, rorder, rstride, -1, wekws::kFsmnMemFirTile);
    bad = launch_fir<true>(grad_y, grad_x, B, w_left, w_right, a, s) != 0;
  }
  if (!bad && grad_w_left) {
    const FsmnMemArgs a = make_args(T, D, lorder, lstride, rorder, rstride, +1, wekws::kFsmnMemGradTile);
    const int64_t tiles = wekws::fsmn_memory_grad_tiles(B, T);
    const unsigned chblocks = unsigned((D + wekws::kFsmnMemChannels - 1) / wekws::kFsmnMemChannels);
    const size_t lds = size_t(wekws::fsmn_memory_grad_lds_bytes(a.halo + 1));
    double* ws = static_cast<double*>(workspace);
    if (can_vec(D, x, grad_y))
      hipLaunchKernelGGL((wekws::fsmn_memory_tap_grad_kernel<4>), dim3(unsigned(tiles), chblocks), dim3(wekws::kFsmnMemThreads), lds, s, x,
                         grad_y, ws, a);
    else
      hipLaunchKernelGGL((wekws::fsmn_memory_tap_grad_kernel<1>), dim3(unsigned(tiles), chblocks), dim3(wekws::kFsmnMemThreads), lds, s, x,
                         grad_y, ws, a);
    bad = hipGetLastError() != hipSuccess;
    if (!bad) {
      hipLaunchKernelGGL(wekws::fsmn_memory_fold_kernel, dim3(unsigned(lorder + rorder), chblocks), dim3(wekws::kFsmnMemThreads), 0, s,
                         static_cast<const double*>(ws), tiles, D, lorder, rorder, grad_w_left, grad_w_right);
      bad = hipGetLastError() != hipSuccess;
    }
  }
  if (bad) return fail(WEKWS_HIP_EDEVICE, "fsmn_memory_backward launch failed");
  return WEKWS_HIP_OK;
}

}  // extern "C"
