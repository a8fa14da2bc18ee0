// Counter-based normal noise for the dithered front end (fbank.hip.h, DITHER): Philox4x32-10 + Box-Muller.
//
// The reference adds  frame[i] += dither * N(0, 1)  after framing and before DC removal (torchaudio.compliance.kaldi._get_window;
// runtime/core/frontend/fbank.h:150-153), an independent draw per (frame, sample), from a sequential host generator.  Here the draw
// at (seed, row id, frame, sample) is a PURE FUNCTION of those four numbers -- no state, no HBM traffic, the same value whatever the
// batch, the grid, the lane that asks or the sample type.  THE definition (restated in tests/dither_ref.py, the oracle):
//
//   generator  Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
//   key        (seed & 0xffffffff, seed >> 32)
//   counter    (block within the frame, frame index, row id & 0xffffffff, row id >> 32)
//   mapping    sample i of a frame belongs to the sample pair n = i >> 1; pair n is served by
//                  block  c0 = (n & 63) | ((n >> 7) << 6)      -- the fbank lane l = n & 63 holds the pairs l + 64 m, m = 0 .. 3:
//                  words  w = 2 ((n >> 6) & 1)  and  w + 1        block l + 64 j serves its pairs m = 2 j and 2 j + 1, so a lane
//                                                                 draws two blocks per frame and uses every word of both
//   uniforms   u = (2 (word >> 9) + 1) 2^-24: an odd multiple of 2^-24 inside (0, 1) with 24 significant bits, exact in float32,
//              so a float64 oracle starts from the same numbers (u1 from word w, u2 from word w + 1).  The smallest is 2^-24:
//              |z| reaches sqrt(48 ln 2) = 5.77.  (((word >> 8) + 0.5) 2^-24 needs 25 bits above 1/2: not a float32.)
//   normals    r = sqrt(-2 ln u1);  sample 2 n gets r cos(2 pi u2), sample 2 n + 1 gets r sin(2 pi u2)
//
// Arithmetic: every step is written as single operations and explicit fused multiply-adds (nothing for the compiler to contract one
// way in one kernel and another way in the next), so the feature kernels and wekws_hip_dither_noise produce the same bits.
//   * -2 ln u: the exponent split off, ln m = 2 atanh((m - 1) / (m + 1)) as a polynomial on [sqrt(1/2), sqrt(2)) -- relative
//     accuracy near u = 1 too, where v_log_f32 times ln 2 is only absolutely accurate (r is small there: its error would be 1e-4);
//   * the angle is reduced in INTEGER arithmetic: u2 = j 2^-24, the nearest quarter turn is (j + 2^21) >> 22 and what is left,
//     f in (-1/2, 1/2) quarter turns, is exact; sin and cos of f pi / 2 are polynomials in f.  (v_sin_f32 / v_cos_f32 take
//     revolutions too but are accurate to about 2^-21 absolute: 8 units of the test's bar per unit of r.)
// Measured against the float64 oracle in units of 2^-24 max(1, |z|): tests/test_hip_dither.py (the bar: K_NOISE_Z).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wekws {

struct PhiloxWords { uint32_t w[4]; };

__host__ __device__ __forceinline__ PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = uint64_t(0xD2511F53u) * c0;
    const uint64_t p1 = uint64_t(0xCD9E8D57u) * c2;
    const uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = uint32_t(p0 >> 32) ^ c3 ^ k1;
    c1 = uint32_t(p1);
    c3 = uint32_t(p0);
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return PhiloxWords{{c0, c1, c2, c3}};
}

// block within the frame that serves sample pair n, and the first of the pair's two words
__host__ __device__ __forceinline__ int philox_pair_block(int n) { return (n & 63) | ((n >> 7) << 6); }
__host__ __device__ __forceinline__ int philox_pair_word(int n) { return 2 * ((n >> 6) & 1); }

// -2 ln u for u = j 2^-24, j = 2 (word >> 9) + 1
__device__ __forceinline__ float philox_neg2ln(uint32_t word) {
  const float u = float(2u * (word >> 9) + 1u) * 5.9604644775390625e-08f;                  // exact
  const float m0 = __builtin_amdgcn_frexp_mantf(u);                                         // [0.5, 1)
  const bool low = m0 < 0.70710678f;
  const float m = low ? 2.f * m0 : m0;                                                      // [sqrt(1/2), sqrt(2))
  const float k = float(__builtin_amdgcn_frexp_expf(u) - int(low));
  const float num = m - 1.f;                                                                // exact
  const float den = m + 1.f;
  const float rc = __builtin_amdgcn_rcpf(den);
  float s = num * rc;
  s = fmaf(fmaf(-den, s, num), rc, s);                                                      // one Newton step: (m - 1) / (m + 1) to half an ulp
  const float p = s * s;                                                                    // <= 0.0295
  float q = fmaf(p, 0.0909090909f, 0.111111111f);                                           // atanh s = s (1 + p / 3 + p^2 / 5 + p^3 / 7 + p^4 / 9 + p^5 / 11)
  q = fmaf(p, q, 0.142857143f);
  q = fmaf(p, q, 0.2f);
  q = fmaf(p, q, 0.333333333f);
  q = q * p;
  const float s4 = -4.f * s;
  const float lm = fmaf(s4, q, s4);                                                         // -2 ln m
  return fmaf(k, -1.38629436f, fmaf(k, 3.80930842e-9f, lm));                                // -2 ln 2 = -1.38629436111989057 = -1.3862943649291992 + 3.8093084e-9
}

// (cos, sin) of 2 pi u for u = j 2^-24, j = 2 (word >> 9) + 1
__device__ __forceinline__ float2 philox_cossin(uint32_t word) {
  const int j = int(2u * (word >> 9) + 1u);                                                 // odd, 1 .. 2^24 - 1
  const int quad = (j + (1 << 21)) >> 22;                                                   // nearest quarter turn, 0 .. 4
  const float f = float(j - (quad << 22)) * 2.384185791015625e-07f;                          // quarter turns left, (-1/2, 1/2): exact
  const float p = f * f;
  // sin(f pi / 2) = f (a1 + a3 p + a5 p^2 + a7 p^3 + a9 p^4), a_k = (+-)(pi / 2)^k / k!
  float sp = fmaf(p, 1.60441185e-4f, -4.68175413e-3f);
  sp = fmaf(p, sp, 7.96926262e-2f);
  sp = fmaf(p, sp, -6.45964098e-1f);
  sp = sp * p;
  const float fa = f * 1.57079637f;
  float s = fmaf(f, -4.37113883e-8f, fa);                                                    // f pi / 2 with pi / 2 = 1.57079637 - 4.37113883e-8
  s = fmaf(f, sp, s);                                                                        // + f (a3 p + a5 p^2 + ...)
  // cos(f pi / 2) = 1 + b2 p + b4 p^2 + b6 p^3 + b8 p^4 + b10 p^5
  float cp = fmaf(p, -2.52020424e-5f, 9.19260275e-4f);
  cp = fmaf(p, cp, -2.08634808e-2f);
  cp = fmaf(p, cp, 2.53669508e-1f);
  cp = fmaf(p, cp, -1.23370055f);
  const float c = fmaf(p, cp, 1.f);
  // quarter turn q: (cos, sin)(q pi / 2 + x) = (c, s), (-s, c), (-c, -s), (s, -c)
  const bool swap = quad & 1;
  float rc = swap ? s : c;
  float rs = swap ? c : s;
  rc = ((quad + 1) & 2) ? -rc : rc;
  rs = (quad & 2) ? -rs : rs;
  return make_float2(rc, rs);
}

// the two normals of a word pair: (sample 2 n, sample 2 n + 1)
__device__ __forceinline__ float2 philox_normal_pair(uint32_t wa, uint32_t wb) {
  const float r = __builtin_amdgcn_sqrtf(philox_neg2ln(wa));                                // (the argument is a normal float in [1.1e-7, 33.3])
  const float2 cs = philox_cossin(wb);
  return make_float2(r * cs.x, r * cs.y);
}

// the generator of a launch: key and the (uniform) high counter words are set per frame by the caller
struct PhiloxDither {
  uint32_t k0, k1;
  __device__ __forceinline__ void init(uint64_t seed) { k0 = uint32_t(seed); k1 = uint32_t(seed >> 32); }
  // the normals of the sample pairs n and n + 64 (n = l + 128 j: one block) of frame `frame` of row `row`
  __device__ __forceinline__ void block(int n, int frame, int64_t row, float2& za, float2& zb) const {
    const PhiloxWords x = philox4x32_10(uint32_t(philox_pair_block(n)), uint32_t(frame), uint32_t(uint64_t(row)), uint32_t(uint64_t(row) >> 32), k0, k1);
    za = philox_normal_pair(x.w[0], x.w[1]);
    zb = philox_normal_pair(x.w[2], x.w[3]);
  }
};

}  // namespace wekws
