// Streaming threshold detector for max-pooling models, many streams at once: the alarm scan of wekws/bin/compute_det.py:89-96
//   i = 0; while i < len: if score[i] >= th: n += 1, i += window_shift  else i += 1
// carried across chunks, per stream and per keyword (each keyword on its own).  With a = the frame's index since the stream's
// reset, the state of a (stream, keyword) is
//   seen        frames consumed so far (the a of the next chunk's first frame)
//   resume      the first frame the scan looks at again: a frame FIRES iff a >= resume and double(score) >= threshold[k] -- the
//               comparison of det_alarm_kernel<false> (det.hip.h); a NaN never fires -- and then resume = a + window_shift
//   best, best_frame   the running maximum since reset and its first frame (ties -> lowest frame, NaN ignored, as
//               det_maxpool_kernel); -inf / -1 before any frame
// so for any split of a score sequence into chunks, empty ones included, the fired frames are those of one scan over the whole.
//
// One thread per (row, keyword): a chunk is tens of frames and inherently serial, the streams are the parallelism.  The kernel
// bounds every index by itself: a row whose frame count lies outside 0..Tcap, whose id lies outside the pool or whose frame
// index would pass int32 is skipped untouched -- its outputs get the fill values, its status word says why -- and hits are
// written only below Dcap = ceil(Tcap / window_shift), which a chunk of Tcap frames cannot exceed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wekws {

struct ThresholdSlot {      // state of one (stream, keyword)
  int32_t seen, resume, best_frame;
  float best;
};

struct ThresholdParams {
  int32_t K, window_shift, n_streams;
  const double* thresholds;   // (K) device
  ThresholdSlot* slots;       // (n_streams, K) device
};

constexpr int kThresholdBadCount = 1, kThresholdBadId = 2, kThresholdFrameRange = 3;   // status words of a skipped row

__device__ __forceinline__ void threshold_slot_clear(ThresholdSlot& s) {
  s.seen = 0; s.resume = 0; s.best_frame = -1; s.best = -INFINITY;
}

__global__ __launch_bounds__(256) void threshold_kws_step_kernel(const ThresholdParams p, const float* __restrict__ probs, int B,
                                                                 int Tcap, int Dcap, const int32_t* __restrict__ ids,
                                                                 const int32_t* __restrict__ frames,
                                                                 int32_t* __restrict__ hit_frames, float* __restrict__ hit_scores,
                                                                 float* __restrict__ best, int32_t* __restrict__ best_frame,
                                                                 int32_t* __restrict__ status) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;             // e = row * K + keyword
  if (e >= int64_t(B) * p.K) return;
  const int b = int(e / p.K), k = int(e - int64_t(b) * p.K);
  const int n = frames ? frames[b] : Tcap;
  const int id = ids[b];
  int32_t* const hf = hit_frames + e * Dcap;
  float* const hs = hit_scores + e * Dcap;
  int st = 0;
  if (n < 0 || n > Tcap) st = kThresholdBadCount;
  else if (id < 0 || id >= p.n_streams) st = kThresholdBadId;
  ThresholdSlot s;
  threshold_slot_clear(s);
  if (!st) {
    s = p.slots[int64_t(id) * p.K + k];
    // a + window_shift must stay an int32 for every frame of the chunk (two and a half centuries of 10 ms frames away)
    if (s.seen < 0 || int64_t(s.seen) + n + p.window_shift > 0x7fffffffLL) st = kThresholdFrameRange;
  }
  int hits = 0;
  if (!st) {
    const double th = p.thresholds[k];
    const float* const x = probs + int64_t(b) * Tcap * p.K + k;
    for (int t = 0; t < n; ++t) {
      const float v = x[int64_t(t) * p.K];
      const int a = s.seen + t;
      if (v > s.best) { s.best = v; s.best_frame = a; }                    // (strict: the first frame of a tie stays; NaN: false)
      if (a >= s.resume && double(v) >= th) {
        if (hits < Dcap) { hf[hits] = a; hs[hits] = v; }
        ++hits;
        s.resume = a + p.window_shift;
      }
    }
    s.seen += n;
    p.slots[int64_t(id) * p.K + k] = s;
  }
  for (int i = hits < Dcap ? hits : Dcap; i < Dcap; ++i) { hf[i] = -1; hs[i] = 0.f; }
  best[e] = s.best;
  best_frame[e] = s.best_frame;
  if (status && k == 0) status[b] = st;
}

__global__ __launch_bounds__(256) void threshold_kws_reset_kernel(const ThresholdParams p, const int32_t* __restrict__ ids, int n) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;             // e = entry of ids * K + keyword; ids NULL: every stream
  if (e >= int64_t(n) * p.K) return;
  const int i = int(e / p.K), k = int(e - int64_t(i) * p.K);
  const int id = ids ? ids[i] : i;
  if (id < 0 || id >= p.n_streams) return;
  threshold_slot_clear(p.slots[int64_t(id) * p.K + k]);
}

int launch_threshold_kws_step(const ThresholdParams& p, const float* probs, int B, int Tcap, int Dcap, const int32_t* ids,
                              const int32_t* frames, int32_t* hit_frames, float* hit_scores, float* best, int32_t* best_frame,
                              int32_t* status, hipStream_t stream);
int launch_threshold_kws_reset(const ThresholdParams& p, const int32_t* ids, int n, hipStream_t stream);

}  // namespace wekws
