// The host plan of the augmentation stages: add_reverb, add_noise and spec_aug of wekws/dataset/processor.py (lines 374-392,
// 395-430, 206-240).  Pure host C++, no HIP: block and partition counts, workspace sizes, the RIR's normalisation and partition
// spectra, and the check every call makes of its per-row tables before anything is launched.
//
// Reverberation is the causal FIR  y[n] = sum_{k=0..min(n, L-1)} h[k] x[n-k],  h = rir / sqrt(sum rir^2),  n < len(x),  as
// overlap-save convolution with the RIR in uniform partitions:
//   H = 2048 (the hop), N = 2H (the transform);  partition p of an L-tap RIR is h[pH .. (p+1)H) behind H zeros' worth of room,
//   P = ceil(L / H) of them;  a row of n samples has ceil(n / H) blocks;
//   X[b]   = FFT_N(x[(b-1)H .. (b+1)H)),  zeros before sample 0 and from sample n on;       Hf[p] = FFT_N(partition p)
//   y[bH .. (b+1)H) = the last H samples of IFFT_N(sum_{p=0..min(P-1, b)} X[b-p] Hf[p])
// Both spectra are of real signals: bins 0..H are kept, (H + 1) complex each.
#pragma once
#include <stdint.h>

#include <cmath>
#include <complex>
#include <vector>

namespace wekws {

constexpr int kReverbHop = 2048;                 // H
constexpr int kReverbFft = 2 * kReverbHop;       // N
constexpr int kReverbBins = kReverbHop + 1;      // bins kept of a real signal's spectrum
constexpr int kAugmentMaxLen = 0x3fffffff;       // longest row / RIR / noise, in samples

inline int64_t reverb_partitions(int64_t L) { return (L + kReverbHop - 1) / kReverbHop; }
inline int64_t reverb_blocks(int64_t n) { return (n + kReverbHop - 1) / kReverbHop; }
// bytes of the partition spectra of an L-tap RIR on the device
inline int64_t reverb_spectra_bytes(int64_t L) { return reverb_partitions(L) * kReverbBins * 8; }
// bytes of the scratch of one call: the input spectra of B rows of up to nmax samples, then one flag per row
inline int64_t reverb_flags_offset(int64_t B, int64_t nmax) { return B * reverb_blocks(nmax) * kReverbBins * 8; }
inline int64_t reverb_workspace_bytes(int64_t B, int64_t nmax) { return reverb_flags_offset(B, nmax) + ((B * 4 + 15) / 16) * 16; }

// ---- what a call is refused for; `row` receives the offending row.  0 = fine.
enum AugmentRefusal {
  kAugOk = 0, kAugBadShape, kAugBadLength, kAugBadIndex, kAugBadStart, kAugBadSnr, kAugBadScale, kAugBadMask
};

inline int reverb_check(const int32_t* rir_len, int R, int B, int nmax, const int32_t* nsamp, const int32_t* rir_of_row, int* row) {
  *row = -1;
  if (B < 0 || nmax < 0 || nmax > kAugmentMaxLen || R < 1 || !rir_len || (B > 0 && !rir_of_row)) return kAugBadShape;
  if (int64_t(B) * reverb_blocks(nmax) > 0x7fffffffLL) return kAugBadShape;
  for (int b = 0; b < B; ++b) {
    *row = b;
    const int n = nsamp ? nsamp[b] : nmax;
    if (n < 0 || n > nmax) return kAugBadLength;
    if (rir_of_row[b] < -1 || rir_of_row[b] >= R) return kAugBadIndex;
  }
  *row = -1;
  return kAugOk;
}

inline int noise_check(const int32_t* noise_len, int Rn, int B, int nmax, const int32_t* nsamp, const int32_t* noise_of_row,
                       const int32_t* start, const double* snr_db, double pcm_scale, int* row) {
  *row = -1;
  if (B < 0 || nmax < 0 || nmax > kAugmentMaxLen || Rn < 1 || !noise_len || (B > 0 && (!noise_of_row || !start || !snr_db)))
    return kAugBadShape;
  if (!(pcm_scale > 0.0) || !std::isfinite(pcm_scale)) return kAugBadScale;
  for (int b = 0; b < B; ++b) {
    *row = b;
    const int n = nsamp ? nsamp[b] : nmax;
    if (n < 0 || n > nmax) return kAugBadLength;
    const int r = noise_of_row[b];
    if (r < -1 || r >= Rn) return kAugBadIndex;
    if (r < 0) continue;
    if (start[b] < 0) return kAugBadStart;
    // a noise longer than the row is cut, never wrapped: the reference draws start in [0, nlen - n]
    if (noise_len[r] > n && int64_t(start[b]) + n > noise_len[r]) return kAugBadStart;
    if (!std::isfinite(snr_db[b])) return kAugBadSnr;
  }
  *row = -1;
  return kAugOk;
}

// masks are [start, end) pairs, already clipped: 0 <= start <= end <= the row's frames (time) / F (frequency)
inline int spec_mask_check(int B, int T, int F, const int32_t* lengths, const int32_t* t_masks, int nt, const int32_t* f_masks, int nf,
                           int* row) {
  *row = -1;
  if (B < 0 || T < 0 || F < 0 || nt < 0 || nf < 0 || (B > 0 && ((nt > 0 && !t_masks) || (nf > 0 && !f_masks)))) return kAugBadShape;
  if (int64_t(B) * T * F > (int64_t(1) << 40) || int64_t(B) * (1 + 2 * (int64_t(nt) + nf)) > 0x0fffffffLL) return kAugBadShape;
  for (int b = 0; b < B; ++b) {
    *row = b;
    const int len = lengths ? lengths[b] : T;
    if (len < 0 || len > T) return kAugBadLength;
    for (int i = 0; i < nt; ++i) {
      const int s = t_masks[(int64_t(b) * nt + i) * 2], e = t_masks[(int64_t(b) * nt + i) * 2 + 1];
      if (s < 0 || e < s || e > len) return kAugBadMask;
    }
    for (int i = 0; i < nf; ++i) {
      const int s = f_masks[(int64_t(b) * nf + i) * 2], e = f_masks[(int64_t(b) * nf + i) * 2 + 1];
      if (s < 0 || e < s || e > F) return kAugBadMask;
    }
  }
  *row = -1;
  return kAugOk;
}

// ---- the RIR's side, in double on the host
// 0 = fine, 1 = a non-finite tap, 2 = all taps zero.  scale = 1 / sqrt(sum h^2), the sum in double.
inline int reverb_rir_scale(const float* h, int64_t L, double* scale) {
  double s = 0.0;
  for (int64_t k = 0; k < L; ++k) {
    if (!std::isfinite(h[k])) return 1;
    s += double(h[k]) * double(h[k]);
  }
  if (!(s > 0.0)) return 2;
  *scale = 1.0 / std::sqrt(s);
  return 0;
}

// in-place radix-2 FFT of N = 2^k points in double (forward, e^{-2 pi i jk / N}); w: the N / 2 twiddles
inline void reverb_fft_host(std::vector<std::complex<double>>& a, const std::vector<std::complex<double>>& w) {
  const size_t n = a.size();
  for (size_t i = 1, j = 0; i < n; ++i) {
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  for (size_t len = 2; len <= n; len <<= 1)
    for (size_t i = 0; i < n; i += len)
      for (size_t k = 0; k < len / 2; ++k) {
        const std::complex<double> u = a[i + k], v = a[i + k + len / 2] * w[k * (n / len)];
        a[i + k] = u + v;
        a[i + k + len / 2] = u - v;
      }
}

inline std::vector<std::complex<double>> reverb_twiddles_host() {
  std::vector<std::complex<double>> w(size_t(kReverbFft) / 2);
  const double pi = 3.14159265358979323846;
  for (size_t k = 0; k < w.size(); ++k) w[k] = std::polar(1.0, -2.0 * pi * double(k) / kReverbFft);
  return w;
}

// the partition spectra of one normalised RIR, appended to `out` as P x (H + 1) x (re, im) float32
inline void reverb_rir_spectra(const float* h, int64_t L, double scale, const std::vector<std::complex<double>>& w,
                               std::vector<float>* out) {
  std::vector<std::complex<double>> a(static_cast<size_t>(kReverbFft));
  const int64_t P = reverb_partitions(L);
  for (int64_t p = 0; p < P; ++p) {
    for (int i = 0; i < kReverbFft; ++i) {
      const int64_t k = p * kReverbHop + i;
      a[size_t(i)] = (i < kReverbHop && k < L) ? double(h[k]) * scale : 0.0;
    }
    reverb_fft_host(a, w);
    for (int k = 0; k < kReverbBins; ++k) {
      out->push_back(float(a[size_t(k)].real()));
      out->push_back(float(a[size_t(k)].imag()));
    }
  }
}

}  // namespace wekws
