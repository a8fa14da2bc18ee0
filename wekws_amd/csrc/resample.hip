// Launcher of the single-rate kernel (resample.hip.h) and the C ABI of wekws_hip_resample_*.  The handle and everything a call does
// on the host are the rate bank's, with one S16 member (resample_bank.hip.h, resample_bank.hip).
#include "resample_bank.hip.h"

#include "host_util.h"

namespace wekws {

template <typename In, typename Out>
static int launch_one(const ResampleParams& P, size_t lds, const ResampleRow* rows, const void* x, int64_t xstride, int16_t* hist,
                      void* y, int B, int mcap, int max_grid, hipStream_t stream) {
  // (a capacity of 0 still takes one tile per row: a push without room for output moves the streams' history)
  const int tiles_per_row = mcap > 0 ? (mcap + kResampleTile - 1) / kResampleTile : 1;
  const int64_t total = int64_t(B) * tiles_per_row;
  if (total <= 0) return 0;
  const int64_t grid = total < max_grid ? total : max_grid;
  hipLaunchKernelGGL((resample_kernel<In, Out>), dim3(unsigned(grid)), dim3(kResampleTile), lds, stream, P, rows,
                     static_cast<const In*>(x), xstride, reinterpret_cast<In*>(hist), static_cast<Out*>(y), mcap, tiles_per_row, total);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_resample(const ResampleParams& P, size_t lds, int in_i16, int out_i16, const ResampleRow* rows, const void* x,
                    int64_t xstride, int16_t* hist, void* y, int B, int mcap, int max_grid, hipStream_t stream) {
  if (in_i16) return out_i16 ? launch_one<int16_t, int16_t>(P, lds, rows, x, xstride, hist, y, B, mcap, max_grid, stream)
                             : launch_one<int16_t, float>(P, lds, rows, x, xstride, hist, y, B, mcap, max_grid, stream);
  // (float rows have no history: the one-shot entry points alone take them)
  return out_i16 ? launch_one<float, int16_t>(P, lds, rows, x, xstride, nullptr, y, B, mcap, max_grid, stream)
                 : launch_one<float, float>(P, lds, rows, x, xstride, nullptr, y, B, mcap, max_grid, stream);
}

}  // namespace wekws

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

int64_t wekws_hip_resample_num_samples(int orig_freq, int new_freq, int64_t nsamp) {
  if (orig_freq <= 0 || new_freq <= 0 || nsamp < 0) {
    fail(WEKWS_HIP_EINVAL, "resample_num_samples: orig_freq=%d new_freq=%d nsamp=%lld", orig_freq, new_freq, (long long)nsamp);
    return -1;
  }
  wekws::ResamplePlan p;
  const int64_t g = wekws::resample_gcd(orig_freq, new_freq);
  p.o = int32_t(orig_freq / g); p.n = int32_t(new_freq / g);
  return wekws::resample_num_samples(p, nsamp);
}

int wekws_hip_resample_create(const wekws_hip_resample_cfg* cfg, void** out) {
  return wekws::resample_create(wekws_hip_resample::kSingle, cfg, cfg ? &cfg->orig_freq : nullptr, nullptr, 1, out);
}

void wekws_hip_resample_destroy(void* h) { wekws::resample_destroy(h); }

int wekws_hip_resample_max_out(void* h, int nmax, int flush) { return wekws::resample_max_out(h, nmax, flush); }

// one-shot: every row an utterance of nsamp[b] samples (NULL: nmax) from its first sample
int wekws_hip_resample_compute(void* h, const float* pcm, int B, int nmax, const int32_t* nsamp, void* out, int mcap, void* stream) {
  return wekws::resample_compute(h, wekws::kResampleBankF32, pcm, B, nmax, nsamp, nullptr, out, mcap, stream);
}

int wekws_hip_resample_compute_i16(void* h, const int16_t* pcm, int B, int nmax, const int32_t* nsamp, void* out, int mcap,
                                   void* stream) {
  return wekws::resample_compute(h, wekws::kResampleBankI16, pcm, B, nmax, nsamp, nullptr, out, mcap, stream);
}

int wekws_hip_resample_push(void* h, const int16_t* pcm, int B, int nmax, const int32_t* stream_ids, const int32_t* nsamp, int flush,
                            void* out, int mcap, int32_t* counts, void* stream) {
  return wekws::resample_push(h, 0, pcm, B, nmax, stream_ids, nsamp, flush, out, mcap, counts, stream);
}

int wekws_hip_resample_reset(void* h, const int32_t* ids, int n) { return wekws::resample_reset(h, ids, n, nullptr); }

int wekws_hip_resample_counts(void* h, int id, int64_t counts_out[4]) { return wekws::resample_counts(h, id, counts_out); }

}  // extern "C"
