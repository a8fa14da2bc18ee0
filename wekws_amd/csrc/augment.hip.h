// The augmentation stages on the device (augment_plan.h states the definitions): reverberation as partitioned overlap-save
// convolution, the noise mix at a drawn SNR, the SpecAugment masks.
//
// Reverberation, two kernels over the (row, block) grid, 256 lanes a workgroup, persistent:
//   reverb_forward_kernel   block b of a row: the 2H samples x[(b-1)H .. (b+1)H) (zeros outside [0, n)) as complex numbers in
//                           LDS, a 4096-point radix-4 decimation-in-frequency transform in place (two passes at a time in
//                           registers: reverb_fft_step), bins 0..H to the scratch.  The
//                           sum of squares of the samples, in double, is reduced on the way: a block whose energy is not
//                           finite holds a NaN or an Inf, and flags its row.
//   reverb_inverse_kernel   block b of a row: sum_{p = 0..min(P-1, b)} X[b-p] Hf[p], p ascending, fmaf in f32, one lane a bin;
//                           the bin and its mirror go to their digit-reversed places in LDS, a decimation-in-time transform
//                           with the conjugate twiddles brings them back in natural order, the last H samples / N are the
//                           block.  A flagged row is NaN over its n samples; a row without an RIR is copied bit for bit.
//   The forward transform leaves bin k at the base-4 digit reversal of k and the inverse takes it from there: neither reorders.
//   LDS: 4096 complex + the 1024 twiddles e^{-2 pi i k / 4096} of the first quadrant (the passes need three quadrants: a quarter
//   turn is a swap and a sign), one element of padding behind every 16: 42.5 KB, three workgroups a CU.
//   Every (row, block) is computed by one workgroup from that row's samples alone, in a fixed order: a row's result does not
//   depend on the batch, and two calls give the same bits.
//   Plain f32 arithmetic on scalars: the unit is built with -fno-slp-vectorize, so that no packed-f32 instruction is formed
//   (pk_safe.hip.h; tests/test_isa_hazard.py scans what was built).
//
// Noise mix, one workgroup a row: both mean squares in double (strided partial sums, a fixed tree), the gain in double by lane
// 0, rounded to f32, then out = fmaf(pcm_scale g, v, pcm).  Masks: one lane an element.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "augment_plan.h"

namespace wekws {

constexpr int kAugThreads = 256;
constexpr int kReverbTwiddles = kReverbFft / 4;     // e^{-2 pi i k / N} of the first quadrant; the passes need k < 3N/4

struct __attribute__((aligned(8))) AugC { float x, y; };     // a complex number; scalar members on purpose (no vector type, no packed arithmetic)

struct ReverbRow {
  int32_t n;          // valid samples
  int32_t nblk;       // ceil(n / H)
  int32_t part_off;   // first partition of the row's RIR in the bank
  int32_t P;          // its partitions; 0: no RIR, the row is copied
};

struct NoiseRow {
  int64_t off;        // first sample of the row's noise in the bank
  int32_t n;          // valid samples
  int32_t nlen;       // samples of the noise; 0: no noise, the row is copied
  int32_t start;      // 0 <= start < nlen
  int32_t reserved;
  double snr_db;
};

__host__ __device__ __forceinline__ AugC aug_cmul(AugC a, AugC w) {
  return AugC{fmaf(a.x, w.x, -(a.y * w.y)), fmaf(a.x, w.y, a.y * w.x)};
}
__host__ __device__ __forceinline__ AugC aug_cmul_conj(AugC a, AugC w) {       // a conj(w)
  return AugC{fmaf(a.x, w.x, a.y * w.y), fmaf(a.y, w.x, -(a.x * w.y))};
}

// base-4 digit reversal of a 12-bit index: digits 0 <-> 5, 1 <-> 4, 2 <-> 3
__host__ __device__ __forceinline__ int reverb_rev(int k) {
  return ((k & 0x003) << 10) | ((k & 0x00c) << 6) | ((k & 0x030) << 2) | ((k >> 2) & 0x030) | ((k >> 6) & 0x00c) | ((k >> 10) & 0x003);
}

// LDS layout: one element of padding behind every 16, for the data and for the twiddles alike.  A lane of a radix-16 pass holds
// 16 elements q apart; with q = 256, 16 and 1 the padded addresses of a wave's 64 lanes spread over all 32 eight-byte banks,
// where the plain layout puts the q = 1 pass on two of them.
__host__ __device__ __forceinline__ int reverb_pad(int i) { return i + (i >> 4); }
constexpr int kReverbLdsData = kReverbFft + kReverbFft / 16;
constexpr int kReverbLdsTwiddles = kReverbTwiddles + kReverbTwiddles / 16;
constexpr size_t kReverbLdsBytes = size_t(kReverbLdsData + kReverbLdsTwiddles) * 8;

// e^{-2 pi i k / N}, k < 3N/4, from the first quadrant's table: a quarter turn further is a multiplication by -i
static_assert(kReverbTwiddles == 1024, "reverb_twiddle takes the quadrant from bit 10");
__host__ __device__ __forceinline__ AugC reverb_twiddle(const AugC* tw, int k) {
  const AugC w = tw[reverb_pad(k & (kReverbTwiddles - 1))];
  const int turn = k >> 10;
  return turn == 0 ? w : turn == 1 ? AugC{w.y, -w.x} : AugC{-w.x, -w.y};
}

// One radix-4 butterfly of a pass over blocks of M points: forward, decimation in frequency (butterfly, then the twiddles
// w^j, w^2j, w^3j of the block); inverse, its transpose conjugate (conjugate twiddles, then the butterfly with +i).
template <bool kInverse>
__host__ __device__ __forceinline__ void reverb_bfly4(AugC& a0, AugC& a1, AugC& a2, AugC& a3, AugC w1, AugC w2, AugC w3) {
  if (kInverse) { a1 = aug_cmul_conj(a1, w1); a2 = aug_cmul_conj(a2, w2); a3 = aug_cmul_conj(a3, w3); }
  const AugC t0{a0.x + a2.x, a0.y + a2.y}, t1{a0.x - a2.x, a0.y - a2.y}, t2{a1.x + a3.x, a1.y + a3.y};
  const AugC dd{a1.x - a3.x, a1.y - a3.y};
  const AugC t3 = kInverse ? AugC{-dd.y, dd.x} : AugC{dd.y, -dd.x};          // +i d : -i d
  a0 = AugC{t0.x + t2.x, t0.y + t2.y}; a1 = AugC{t1.x + t3.x, t1.y + t3.y};
  a2 = AugC{t0.x - t2.x, t0.y - t2.y}; a3 = AugC{t1.x - t3.x, t1.y - t3.y};
  if (!kInverse) { a1 = aug_cmul(a1, w1); a2 = aug_cmul(a2, w2); a3 = aug_cmul(a3, w3); }
}

// Two radix-4 passes in registers: the passes over blocks of M = 16 q and of M / 4 points touch, for one j < q, the same 16
// elements q apart.  A lane loads them, makes both passes (forward: M then M / 4; inverse: M / 4 then M) and stores them: three
// trips through LDS per transform instead of six.  The three forward steps q = 256, 16, 1 take natural order to base-4
// digit-reversed, the three inverse steps q = 1, 16, 256 take it back, scaled by N.  d, tw: padded (reverb_pad);
// tw: the first quadrant's twiddles (reverb_twiddle).
template <bool kInverse>
__host__ __device__ __forceinline__ void reverb_fft_step(AugC* d, const AugC* tw, int log2q, int lane, int lanes) {
  const int q = 1 << log2q, M = q << 4, tws = kReverbFft / M;
  for (int i = lane; i < kReverbFft / 16; i += lanes) {
    const int blk = i >> log2q, j = i & (q - 1), base = blk * M + j;
    AugC e[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) e[m] = d[reverb_pad(base + m * q)];
    const AugC v1 = reverb_twiddle(tw, 4 * j * tws), v2 = reverb_twiddle(tw, 8 * j * tws), v3 = reverb_twiddle(tw, 12 * j * tws);
    if (kInverse) {
#pragma unroll
      for (int k = 0; k < 4; ++k) reverb_bfly4<true>(e[4 * k], e[4 * k + 1], e[4 * k + 2], e[4 * k + 3], v1, v2, v3);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int ja = (j + m * q) * tws;
      reverb_bfly4<kInverse>(e[m], e[m + 4], e[m + 8], e[m + 12], reverb_twiddle(tw, ja), reverb_twiddle(tw, 2 * ja), reverb_twiddle(tw, 3 * ja));
    }
    if (!kInverse) {
#pragma unroll
      for (int k = 0; k < 4; ++k) reverb_bfly4<false>(e[4 * k], e[4 * k + 1], e[4 * k + 2], e[4 * k + 3], v1, v2, v3);
    }
#pragma unroll
    for (int m = 0; m < 16; ++m) d[reverb_pad(base + m * q)] = e[m];
  }
}

__device__ __forceinline__ void reverb_fft_forward(AugC* d, const AugC* tw, int tid) {
  for (int lq = 8; lq >= 0; lq -= 4) {
    reverb_fft_step<false>(d, tw, lq, tid, kAugThreads);
    __syncthreads();
  }
}
__device__ __forceinline__ void reverb_fft_inverse(AugC* d, const AugC* tw, int tid) {
  for (int lq = 0; lq <= 8; lq += 4) {
    reverb_fft_step<true>(d, tw, lq, tid, kAugThreads);
    __syncthreads();
  }
}

// X: (B, nbmax, H + 1) complex; bad: (B) flags, zeroed before the launch
__global__ __launch_bounds__(kAugThreads) void reverb_forward_kernel(const ReverbRow* __restrict__ rows, const float* __restrict__ pcm,
                                                                     int nmax, int nbmax, const AugC* __restrict__ twiddles,
                                                                     AugC* __restrict__ X, int32_t* __restrict__ bad, int64_t total) {
  extern __shared__ __attribute__((aligned(16))) unsigned char augment_lds[];
  AugC* const d = reinterpret_cast<AugC*>(augment_lds);
  AugC* const tw = d + kReverbLdsData;
  const int tid = threadIdx.x;
  for (int e = tid; e < kReverbTwiddles; e += kAugThreads) tw[reverb_pad(e)] = twiddles[e];
  for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
    const int row = int(t / nbmax), blk = int(t - int64_t(row) * nbmax);
    const ReverbRow R = rows[row];
    if (R.P == 0 || blk >= R.nblk) continue;                       // (the whole workgroup)
    const float* const x = pcm + int64_t(row) * nmax;
    const int lo = (blk - 1) * kReverbHop;
    double energy = 0.0;
    for (int i = tid; i < kReverbFft; i += kAugThreads) {
      const int pos = lo + i;
      const float v = (pos >= 0 && pos < R.n) ? x[pos] : 0.f;
      d[reverb_pad(i)] = AugC{v, 0.f};
      energy = fma(double(v), double(v), energy);
    }
    // (squares of f32 cannot overflow a double: the sum is non-finite exactly when a sample is)
    const bool nonfinite = (__double_as_longlong(energy) & 0x7ff0000000000000LL) == 0x7ff0000000000000LL;
    if (__syncthreads_or(nonfinite) && tid == 0) bad[row] = 1;
    reverb_fft_forward(d, tw, tid);
    AugC* const Xb = X + (int64_t(row) * nbmax + blk) * kReverbBins;
    for (int k = tid; k < kReverbBins; k += kAugThreads) Xb[k] = d[reverb_pad(reverb_rev(k))];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kAugThreads) void reverb_inverse_kernel(const ReverbRow* __restrict__ rows, const float* __restrict__ pcm,
                                                                     int nmax, int nbmax, const AugC* __restrict__ twiddles,
                                                                     const AugC* __restrict__ X, const AugC* __restrict__ Hf,
                                                                     const int32_t* __restrict__ bad, float* __restrict__ out,
                                                                     int64_t total) {
  extern __shared__ __attribute__((aligned(16))) unsigned char augment_lds[];
  AugC* const d = reinterpret_cast<AugC*>(augment_lds);
  AugC* const tw = d + kReverbLdsData;
  const int tid = threadIdx.x;
  for (int e = tid; e < kReverbTwiddles; e += kAugThreads) tw[reverb_pad(e)] = twiddles[e];
  __syncthreads();
  for (int64_t t = blockIdx.x; t < total; t += gridDim.x) {
    const int row = int(t / nbmax), blk = int(t - int64_t(row) * nbmax);
    const ReverbRow R = rows[row];
    if (blk >= R.nblk) continue;                                   // (the whole workgroup, as the branches below)
    const int o0 = blk * kReverbHop, cnt = min(kReverbHop, R.n - o0);
    float* const y = out + int64_t(row) * nmax + o0;
    if (R.P == 0) {
      const float* const x = pcm + int64_t(row) * nmax + o0;
      for (int i = tid; i < cnt; i += kAugThreads) y[i] = x[i];
      continue;
    }
    if (bad[row]) {
      for (int i = tid; i < cnt; i += kAugThreads) y[i] = __uint_as_float(0x7fc00000u);
      continue;
    }
    const int pmax = min(R.P - 1, blk);
    const AugC* const Xb = X + (int64_t(row) * nbmax + blk) * kReverbBins;
    const AugC* const Hr = Hf + int64_t(R.part_off) * kReverbBins;
    for (int k = tid; k < kReverbBins; k += kAugThreads) {
      AugC acc{0.f, 0.f};
      for (int p = 0; p <= pmax; ++p) {
        const AugC a = Xb[k - int64_t(p) * kReverbBins], h = Hr[k + int64_t(p) * kReverbBins];
        acc.x = fmaf(a.x, h.x, acc.x); acc.x = fmaf(-a.y, h.y, acc.x);
        acc.y = fmaf(a.x, h.y, acc.y); acc.y = fmaf(a.y, h.x, acc.y);
      }
      d[reverb_pad(reverb_rev(k))] = acc;
      if (k > 0 && k < kReverbHop) d[reverb_pad(reverb_rev(kReverbFft - k))] = AugC{acc.x, -acc.y};
    }
    __syncthreads();
    reverb_fft_inverse(d, tw, tid);
    for (int i = tid; i < cnt; i += kAugThreads) y[i] = d[reverb_pad(kReverbHop + i)].x * (1.f / kReverbFft);
    __syncthreads();
  }
}

// one workgroup a row; out may be pcm
__global__ __launch_bounds__(kAugThreads) void noise_mix_kernel(const NoiseRow* __restrict__ rows, const float* pcm, int nmax,
                                                                const float* __restrict__ bank, float pcm_scale, float* out) {
  __shared__ double part[2][kAugThreads];
  __shared__ float gain;
  const int tid = threadIdx.x;
  const NoiseRow R = rows[blockIdx.x];
  const float* const x = pcm + int64_t(blockIdx.x) * nmax;
  float* const y = out + int64_t(blockIdx.x) * nmax;
  if (R.n <= 0) return;
  if (R.nlen == 0) {
    if (y != x)
      for (int i = tid; i < R.n; i += kAugThreads) y[i] = x[i];
    return;
  }
  const float* const v = bank + R.off;
  const int step = kAugThreads % R.nlen;
  double ea = 0.0, en = 0.0;
  int at = int((int64_t(R.start) + tid) % R.nlen);
  for (int i = tid; i < R.n; i += kAugThreads) {
    const double a = double(x[i]), w = double(v[at]);
    ea = fma(a, a, ea);
    en = fma(w, w, en);
    at += step;
    if (at >= R.nlen) at -= R.nlen;
  }
  part[0][tid] = ea; part[1][tid] = en;
  __syncthreads();
  for (int s = kAugThreads / 2; s > 0; s >>= 1) {
    if (tid < s) { part[0][tid] += part[0][tid + s]; part[1][tid] += part[1][tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    const double adb = 10.0 * log10(part[0][0] / (double(pcm_scale) * double(pcm_scale) * double(R.n)) + 1e-4), ndb = 10.0 * log10(part[1][0] / double(R.n) + 1e-4);
    gain = pcm_scale * float(sqrt(pow(10.0, (adb - ndb - R.snr_db) / 10.0)));
  }
  __syncthreads();
  const float g = gain;
  at = int((int64_t(R.start) + tid) % R.nlen);
  for (int i = tid; i < R.n; i += kAugThreads) {
    y[i] = fmaf(g, v[at], x[i]);
    at += step;
    if (at >= R.nlen) at -= R.nlen;
  }
}

// table: lengths (B) | t_masks (B, nt, 2) | f_masks (B, nf, 2); out may be feats
__global__ __launch_bounds__(kAugThreads) void spec_mask_kernel(const float* feats, int T, int F, const int32_t* __restrict__ table, int B,
                                                                int nt, int nf, float* out, int64_t total) {
  const int32_t* const tm = table + B;
  const int32_t* const fm = tm + int64_t(B) * nt * 2;
  for (int64_t e = int64_t(blockIdx.x) * kAugThreads + threadIdx.x; e < total; e += int64_t(gridDim.x) * kAugThreads) {
    const int64_t fr = e / F;
    const int f = int(e - fr * F), b = int(fr / T), t = int(fr - int64_t(b) * T);
    bool zero = false;
    if (t < table[b]) {
      for (int i = 0; i < nt; ++i) zero |= t >= tm[(int64_t(b) * nt + i) * 2] && t < tm[(int64_t(b) * nt + i) * 2 + 1];
      for (int i = 0; i < nf; ++i) zero |= f >= fm[(int64_t(b) * nf + i) * 2] && f < fm[(int64_t(b) * nf + i) * 2 + 1];
    }
    const float v = feats[e];
    out[e] = zero ? 0.f : v;
  }
}

}  // namespace wekws
