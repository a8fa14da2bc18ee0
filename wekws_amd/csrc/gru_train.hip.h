// The trainable GRU's recurrent scan for gfx950: torch.nn.GRU(batch_first=True)'s time loop of one layer and its backward
// through time, each ONE persistent launch over all T steps.  gru_train_plan.h has the checks, the grid and the sizes.
// The input product gi = W_ih x + b_ih (B, T, 3H) is one large GEMM and stays the caller's; so do the weight, bias and input
// gradients, which are GEMMs and column sums over all (b, t) of the dgi and dgh this file writes.
//
// Decomposition (gru.hip.h's ownership): a workgroup of 8 waves owns 16 batch rows for the whole sequence.  Wave w owns the
// hidden units [16w, 16w+16) of ALL THREE gates, so after the MFMAs lane l holds r, z and q of the same four (unit, row) pairs
// -- units 16w + 4(l>>4) + j, j = 0..3, row l&15 -- and neither the cell nor its gradient needs cross-lane traffic.  Waves
// without a unit tile (w >= H/16) idle through the barriers.  Products are exact float32: v_mfma_f32_16x16x4_f32 with
// A = rows of W_hh and B = an LDS image [k][row] with a row stride of 16 floats.  A wave's A fragments are loaded ONCE per launch
// from the plain row-major (3H, H) parameter tensor and stay in registers (96 per lane at H = 128): the weights change every
// training step, so there is no packed image.  All tensors are batch-major and contiguous; every global access of the time loop
// is a 16-byte access of one lane's four units.
//
//   gru_scan_fwd<H>   h lives in LDS as two images [H][16]; step t reads image t&1 and writes the other, so a step has one
//                     barrier.  gi[:, t+1] is prefetched into registers while step t computes.  Per step and wave: 3 H/4 MFMAs,
//                     the cell, h[t] to LDS and to y[b, t, :], and with a reserve r, z, n, q to reserve[b, t, 0:4H].
//   gru_scan_bwd<H>   t = T-1 .. 0 with the carry in registers (the MFMA result has the lane's own ownership).  Every lane
//                     computes the gate gradients of its pairs, writes dgi[t] and dgh[t] and puts dgh[t] into LDS as [3H][16]
//                     (two images again: one barrier a step); then wave w computes its 16 units of W_hh^T dgh[t] with 3 H/4
//                     MFMAs over the transposed fragments, also loaded once.  The saved tensors of step t-1 are prefetched.
//
// The float32 operation order, the same in every instance.  The object is built with -ffp-contract=off and
// -fno-slp-vectorize: an operation is fused only where fmaf is written, and stays a scalar instruction.
//     a_g   = the MFMA chain over k = 0 .. H-1 ascending from +0, one chain per gate g
//     gh_g  = a_g + b_hh_g                                  (no bias: + 0)
//     r     = 1 / (1 + expf(-(gi_r + gh_r)))                z likewise            q = gh_n
//     n     = tanhf(fmaf(r, q, gi_n))
//     h[t]  = fmaf(z, h[t-1] - n, n)
//   backward, dh = grad_y[t] + carry:
//     dn    = (dh * (1 - z)) * fmaf(-n, n, 1)
//     dz    = ((dh * (h[t-1] - n)) * z) * (1 - z)
//     dq    = dn * r                                        dr = ((dn * q) * r) * (1 - r)
//     dgi   = (dr, dz, dn)                                  dgh = (dr, dz, dq)
//     c_g   = the MFMA chain of W_hh[gH : (g+1)H, u]^T dgh_g over its H rows ascending from +0, one chain per gate
//     carry = fmaf(dh, z, (c_r + c_z) + c_n)
// expf and tanhf are the device library's accurate forms: s saturates to 0 and 1 and tanh to -1 and 1 at +-100 without a NaN,
// and a NaN goes through both.  A row's results depend on that row alone (an MFMA column is a batch row): the same bits in any
// batch position, alone, and on any run.  No floating-point atomics, no waits between workgroups; rows past B compute on zeros
// and store nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gru_train_plan.h"

namespace wekws {

typedef float gru_f32x4 __attribute__((ext_vector_type(4)));

__device__ inline float gru_train_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ inline float4 gru_train_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ inline void gru_train_st4(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ inline void gru_train_unpack(const float4& q, float (&v)[4]) { v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }

template <int H>
__global__ __launch_bounds__(kGruTrainThreads) void gru_scan_fwd(const float* __restrict__ gi, const float* __restrict__ w_hh,
                                                                 const float* __restrict__ b_hh, const float* __restrict__ h0, int B,
                                                                 int T, float* __restrict__ y, float* __restrict__ hn,
                                                                 float* __restrict__ reserve) {
  static_assert(H % 16 == 0 && H >= kGruTrainMinH && H <= kGruTrainMaxH, "the built hidden sizes");
  constexpr int KB = H / 4, SS = kGruTrainStride;
  extern __shared__ __attribute__((aligned(16))) float lds[];          // [2][H][SS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int64_t row = int64_t(blockIdx.x) * kGruTrainRows + l15;
  const bool active = wave < H / 16;
  const bool valid = active && row < B;
  const int u0 = active ? wave * 16 + lq * 4 : 0;                        // first of this lane's 4 hidden units

  // h[-1] <- h0 (or zeros) as [unit][row]
  for (int e = tid; e < kGruTrainRows * H; e += kGruTrainThreads) {
    const int s = e / H, u = e - s * H;
    const int64_t b = int64_t(blockIdx.x) * kGruTrainRows + s;
    lds[u * SS + s] = (h0 && b < B) ? h0[b * H + u] : 0.f;
  }

  // the wave's A fragments: lane holds W_hh[g H + 16 w + l15][4 kb + lq]
  float wa[3][KB];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) wa[g][kb] = active ? w_hh[(int64_t(g) * H + wave * 16 + l15) * H + kb * 4 + lq] : 0.f;
  float bias[3][4];
#pragma unroll
  for (int g = 0; g < 3; ++g) gru_train_unpack(b_hh ? gru_train_ld4(b_hh + g * H + u0) : make_float4(0.f, 0.f, 0.f, 0.f), bias[g]);

  const float* const gi_row = gi + (valid ? row : 0) * int64_t(T) * 3 * H + u0;
  float4 pre[3];
  auto prefetch = [&](int t) {
#pragma unroll
    for (int g = 0; g < 3; ++g)
      pre[g] = (valid && t < T) ? gru_train_ld4(gi_row + int64_t(t) * 3 * H + g * H) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  prefetch(0);
  __syncthreads();

  float hv[4] = {0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < T; ++t) {
    const float* const cur = lds + (t & 1) * H * SS;
    float* const nxt = lds + ((t + 1) & 1) * H * SS;
    float g_r[4], g_z[4], g_n[4];
    gru_train_unpack(pre[0], g_r);
    gru_train_unpack(pre[1], g_z);
    gru_train_unpack(pre[2], g_n);
    prefetch(t + 1);
    if (active) {
      gru_f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, aq = ar;
      const float* const bp = cur + lq * SS + l15;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const float hb = bp[kb * 4 * SS];
        ar = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[0][kb], hb, ar, 0, 0, 0);
        az = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[1][kb], hb, az, 0, 0, 0);
        aq = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[2][kb], hb, aq, 0, 0, 0);
      }
      float rv[4], zv[4], nv[4], qv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float hprev = cur[(u0 + j) * SS + l15];
        rv[j] = gru_train_sigmoid(g_r[j] + (ar[j] + bias[0][j]));
        zv[j] = gru_train_sigmoid(g_z[j] + (az[j] + bias[1][j]));
        qv[j] = aq[j] + bias[2][j];
        nv[j] = tanhf(fmaf(rv[j], qv[j], g_n[j]));
        hv[j] = fmaf(zv[j], hprev - nv[j], nv[j]);
        nxt[(u0 + j) * SS + l15] = hv[j];
      }
      if (valid) {
        const int64_t bt = row * int64_t(T) + t;
        gru_train_st4(y + bt * H + u0, hv);
        if (reserve) {
          float* const rp = reserve + bt * 4 * H + u0;
          gru_train_st4(rp, rv);
          gru_train_st4(rp + H, zv);
          gru_train_st4(rp + 2 * H, nv);
          gru_train_st4(rp + 3 * H, qv);
        }
      }
    }
    __syncthreads();
  }
  if (valid) gru_train_st4(hn + row * H + u0, hv);
}

template <int H>
__global__ __launch_bounds__(kGruTrainThreads) void gru_scan_bwd(const float* __restrict__ grad_y, const float* __restrict__ grad_hn,
                                                                 const float* __restrict__ y, const float* __restrict__ h0,
                                                                 const float* __restrict__ reserve, const float* __restrict__ w_hh,
                                                                 int B, int T, float* __restrict__ grad_gi, float* __restrict__ grad_gh,
                                                                 float* __restrict__ grad_h0) {
  static_assert(H % 16 == 0 && H >= kGruTrainMinH && H <= kGruTrainMaxH, "the built hidden sizes");
  constexpr int KB = H / 4, SS = kGruTrainStride;
  extern __shared__ __attribute__((aligned(16))) float lds[];          // [2][3H][SS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int64_t row = int64_t(blockIdx.x) * kGruTrainRows + l15;
  const bool active = wave < H / 16;
  const bool valid = active && row < B;
  const int u0 = active ? wave * 16 + lq * 4 : 0;

  // the transposed fragments: lane holds W_hh[4 kb + lq][16 w + l15], kb over the 3H rows
  float wt[3][KB];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) wt[g][kb] = active ? w_hh[(int64_t(g) * H + kb * 4 + lq) * H + wave * 16 + l15] : 0.f;

  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float carry[4];
  gru_train_unpack((valid && grad_hn) ? gru_train_ld4(grad_hn + row * H + u0) : zero4, carry);

  // what a step reads: r, z, n, q of step t, h[t-1] and grad_y[t]
  float4 p_r, p_z, p_n, p_q, p_h, p_g;
  auto prefetch = [&](int t) {
    p_r = p_z = p_n = p_q = p_h = p_g = zero4;
    if (valid && t >= 0) {
      const int64_t bt = row * int64_t(T) + t;
      const float* const rp = reserve + bt * 4 * H + u0;
      p_r = gru_train_ld4(rp);
      p_z = gru_train_ld4(rp + H);
      p_n = gru_train_ld4(rp + 2 * H);
      p_q = gru_train_ld4(rp + 3 * H);
      if (t > 0)
        p_h = gru_train_ld4(y + (bt - 1) * H + u0);
      else if (h0)
        p_h = gru_train_ld4(h0 + row * H + u0);
      if (grad_y) p_g = gru_train_ld4(grad_y + bt * H + u0);
    }
  };
  prefetch(T - 1);

  for (int t = T - 1; t >= 0; --t) {
    float* const buf = lds + (t & 1) * 3 * H * SS;
    float rv[4], zv[4], nv[4], qv[4], hp[4], gy[4];
    gru_train_unpack(p_r, rv);
    gru_train_unpack(p_z, zv);
    gru_train_unpack(p_n, nv);
    gru_train_unpack(p_q, qv);
    gru_train_unpack(p_h, hp);
    gru_train_unpack(p_g, gy);
    prefetch(t - 1);
    float dh[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
      float dr[4], dz[4], dn[4], dq[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dh[j] = gy[j] + carry[j];
        const float omz = 1.0f - zv[j];
        dn[j] = (dh[j] * omz) * fmaf(-nv[j], nv[j], 1.0f);
        dz[j] = ((dh[j] * (hp[j] - nv[j])) * zv[j]) * omz;
        dq[j] = dn[j] * rv[j];
        dr[j] = ((dn[j] * qv[j]) * rv[j]) * (1.0f - rv[j]);
        buf[(u0 + j) * SS + l15] = dr[j];
        buf[(H + u0 + j) * SS + l15] = dz[j];
        buf[(2 * H + u0 + j) * SS + l15] = dq[j];
      }
      if (valid) {
        const int64_t o = (row * int64_t(T) + t) * 3 * H + u0;
        gru_train_st4(grad_gi + o, dr);
        gru_train_st4(grad_gi + o + H, dz);
        gru_train_st4(grad_gi + o + 2 * H, dn);
        gru_train_st4(grad_gh + o, dr);
        gru_train_st4(grad_gh + o + H, dz);
        gru_train_st4(grad_gh + o + 2 * H, dq);
      }
    }
    __syncthreads();
    if (active) {
      gru_f32x4 c[3];
      const float* const bp = buf + lq * SS + l15;
#pragma unroll
      for (int g = 0; g < 3; ++g) c[g] = gru_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int g = 0; g < 3; ++g)
          c[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[g][kb], bp[(g * H + kb * 4) * SS], c[g], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) carry[j] = fmaf(dh[j], zv[j], (c[0][j] + c[1][j]) + c[2][j]);
    }
  }
  if (valid && grad_h0) gru_train_st4(grad_h0 + row * H + u0, carry);
}

}  // namespace wekws
