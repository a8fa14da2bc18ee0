// The host plan of the resampler: torchaudio.transforms.Resample(orig, new) with its defaults (sinc_interp_hann,
// lowpass_filter_width 6, rolloff 0.99), the `resample` step of wekws/dataset/processor.py:83-103.  Pure host C++, no HIP:
// the taps, the live range of every phase, the output count and what one push does to one stream.  The kernels
// (resample.hip.h) are told through these numbers alone; so are the host's return values -- no push reads the device.
//
// With g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) rolloff, width = ceil(lpw o / base), K = 2 width + o:
//   t[i][m]  = clamp(((m - width) / o - i / n) base, -lpw, +lpw)                  i = 0..n-1, m = 0..K-1   (float64)
//   k[i][m]  = float32(sinc(pi t) cos^2(pi t / (2 lpw)) base / o)                 sinc(0) = 1
//   y[j n + i] = sum_m k[i][m] x[j o + m - width]                                 x = 0 outside [0, L)
//   len(y)   = ceil(n L / o)
// orig == new is the identity: one phase, one tap of 1.
//
// A tap is LIVE where the clamp is inactive (|t| < lpw).  Where it is active the float64 value is below 2e-49, which float32
// rounds to 0: for finite input, skipping those taps is exact.  t rises with m, so the live taps of a phase are one range
// [first_i, last_i]; both ends rise with i, and first_{0} + o > first_{n-1} (likewise last): over the output index q = j n + i
// the first and the last input sample an output needs are non-decreasing.
//
// Streaming.  Output q is emitted as soon as every live tap of it lies on a received sample:  need(q) = j o + last_i - width + 1
// <= N, N the samples received so far.  need is non-decreasing, so the outputs emitted after N samples are a prefix [0, count(N))
// and count is found by bisection.  A stream keeps the samples from lo(count) = j o + first_i - width of the first output not
// yet emitted: fewer than the live taps of that phase.  Of the received samples, those at or past the position of the first
// output not yet emitted (q o / n) number at most ceil(lpw o / base) + 1 -- the look-ahead of half a filter.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

namespace wekws {

struct ResamplePlan {
  int32_t orig = 0, neu = 0, o = 1, n = 1, lpw = 0, width = 0, K = 1;
  double base = 1.0;
  int32_t max_live = 1;                 // most live taps of a phase
  std::vector<int32_t> first, last;     // live range of every phase (inclusive)
  std::vector<float> taps;              // (n, K), zeros outside the live ranges
};

inline int64_t resample_gcd(int64_t a, int64_t b) {
  while (b) { const int64_t t = a % b; a = b; b = t; }
  return a;
}

// t of tap m of phase i before the clamp, in the reference's order of operations
inline double resample_t(const ResamplePlan& p, int i, int64_t m) {
  return (double(-i) / double(p.n) + double(m - p.width) / double(p.o)) * p.base;
}

inline float resample_tap(const ResamplePlan& p, int i, int64_t m) {
  const double pi = 3.14159265358979323846;
  double t = resample_t(p, i, m);
  const double lim = double(p.lpw);
  t = t < -lim ? -lim : (t > lim ? lim : t);
  const double c = std::cos(t * pi / lim / 2.0);
  const double window = c * c;
  t *= pi;
  const double scale = p.base / double(p.o);
  const double s = t == 0.0 ? 1.0 : std::sin(t) / t;
  return float(s * (window * scale));
}

// The geometry and the live ranges (cheap: no tap is computed).  0, or -1 for rates / parameters no resampler has.
inline int resample_plan_ranges(int orig, int neu, int lpw, double rolloff, ResamplePlan* p) {
  if (orig <= 0 || neu <= 0 || lpw <= 0 || !(rolloff > 0.0) || !(rolloff <= 1.0)) return -1;
  const int64_t g = resample_gcd(orig, neu);
  p->orig = orig; p->neu = neu; p->lpw = lpw;
  p->o = int32_t(orig / g); p->n = int32_t(neu / g);
  if (orig == neu) {
    p->base = 1.0; p->width = 0; p->K = 1; p->max_live = 1;
    p->first.assign(1, 0); p->last.assign(1, 0);
    return 0;
  }
  p->base = double(p->o < p->n ? p->o : p->n) * rolloff;
  const double w = std::ceil(double(lpw) * double(p->o) / p->base);
  if (!(w < 1e9)) return -1;
  p->width = int32_t(w);
  const int64_t K = 2 * int64_t(p->width) + p->o;
  if (K > 0x3fffffffLL) return -1;
  p->K = int32_t(K);
  p->first.resize(size_t(p->n)); p->last.resize(size_t(p->n));
  p->max_live = 1;
  const double lim = double(lpw);
  for (int i = 0; i < p->n; ++i) {
    // a guess from the real-valued bound, settled with the expression the taps themselves use
    const double centre = double(p->width) + double(p->o) * double(i) / double(p->n), half = double(p->o) * lim / p->base;
    int64_t f = int64_t(std::floor(centre - half)) - 2, l = int64_t(std::ceil(centre + half)) + 2;
    if (f < 0) f = 0;
    if (l > K - 1) l = K - 1;
    while (f < K - 1 && !(std::fabs(resample_t(*p, i, f)) < lim)) ++f;
    while (l > f && !(std::fabs(resample_t(*p, i, l)) < lim)) --l;
    p->first[size_t(i)] = int32_t(f); p->last[size_t(i)] = int32_t(l);
    if (l - f + 1 > p->max_live) p->max_live = int32_t(l - f + 1);
  }
  return 0;
}

// ... and the taps: (n, K) float32, computed in double
inline void resample_plan_taps(ResamplePlan* p) {
  p->taps.assign(size_t(p->n) * size_t(p->K), 0.f);
  if (p->orig == p->neu) { p->taps[0] = 1.f; return; }
  for (int i = 0; i < p->n; ++i)
    for (int64_t m = 0; m < p->K; ++m) p->taps[size_t(i) * size_t(p->K) + size_t(m)] = resample_tap(*p, i, m);
}

// ceil(n L / o) without forming n L
inline int64_t resample_num_samples(const ResamplePlan& p, int64_t L) {
  if (L <= 0) return 0;
  const int64_t o = p.o, n = p.n;
  return (L / o) * n + ((L % o) * n + o - 1) / o;
}

// samples that output q needs to have been received: one past its last live tap
inline int64_t resample_need(const ResamplePlan& p, int64_t q) {
  const int64_t j = q / p.n;
  return j * p.o + p.last[size_t(q - j * p.n)] - p.width + 1;
}
// the first sample output q reads (may be negative: zeros in front of the signal)
inline int64_t resample_lo(const ResamplePlan& p, int64_t q) {
  const int64_t j = q / p.n;
  return j * p.o + p.first[size_t(q - j * p.n)] - p.width;
}
// outputs emitted once N samples are in: the first q with need(q) > N
inline int64_t resample_emit_count(const ResamplePlan& p, int64_t N) {
  if (N <= 0) return 0;
  int64_t lo = 0, hi = (N / p.o + 1) * p.n;          // need(hi) > (N / o + 1) o - width + last_0 - width ... > N
  while (resample_need(p, hi) <= N) hi += p.n;        // (never taken: last_i >= width; kept as the proof's belt)
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (resample_need(p, mid) <= N) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct ResampleStep {
  int64_t total;      // outputs emitted once this push is done
  int64_t keep_from;  // the stream keeps samples [keep_from, N + nsamp)
};
// one push of nsamp samples onto a stream that has received N; flush ends the stream with zeros beyond its last sample
inline ResampleStep resample_step(const ResamplePlan& p, int64_t N, int64_t nsamp, int flush) {
  const int64_t N2 = N + nsamp;
  ResampleStep s;
  if (flush) {
    s.total = resample_num_samples(p, N2);
    s.keep_from = N2;
    return s;
  }
  s.total = resample_emit_count(p, N2);
  int64_t k = resample_lo(p, s.total);
  if (k < 0) k = 0;
  if (k > N2) k = N2;
  s.keep_from = k;
  return s;
}
// samples a stream may hold between two pushes (fewer than the live taps of a phase)
inline int32_t resample_hist_cap(const ResamplePlan& p) { return p.max_live; }
// outputs that always suffice for a chunk of up to nmax samples
inline int64_t resample_max_out(const ResamplePlan& p, int64_t nmax, int flush) {
  const int64_t in = nmax + (flush ? int64_t(p.max_live) + 1 : 0);
  return (in * p.n + p.o - 1) / p.o + 2;
}

// ---- what the kernel's launch is sized with (resample.hip.h); host arithmetic, stated here so that a plan of several rates
// (resample_bank_plan.h) can take its maxima without a device header
constexpr int kResampleTile = 256;            // outputs of a tile = lanes of a workgroup
constexpr int kResampleLdsBudget = 64 * 1024; // live table + live ranges + input tile
constexpr int kResampleVec = 8;               // samples of the widest 16-byte group (int16)

// j-blocks that 256 consecutive outputs touch at most
inline int resample_jspan(int n) { return (n + kResampleTile - 2) / n + 1; }
inline int resample_stride(int max_live) { return max_live | 1; }
inline int64_t resample_tile_cap(const ResamplePlan& p) {
  const int64_t c = int64_t(resample_jspan(p.n)) * p.o + 2 * int64_t(p.width) + kResampleVec;
  return (c + kResampleVec - 1) / kResampleVec * kResampleVec;
}
// LDS bytes of a launch with float samples (the larger of the two source types); tile_off if given
inline int64_t resample_lds_bytes(const ResamplePlan& p, int64_t* tile_off = nullptr) {
  int64_t table = (int64_t(p.n) * resample_stride(p.max_live) + 2 * int64_t(p.n)) * 4;
  table = (table + 15) / 16 * 16;
  if (tile_off) *tile_off = table;
  return table + resample_tile_cap(p) * 4;
}

}  // namespace wekws
