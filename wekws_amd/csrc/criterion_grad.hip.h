// The criterion's backward pass on the device: the gradient of wekws/model/loss.py::criterion with respect to its input, in
// closed form from what the forward kernels (criterion.hip.h) compute -- the extreme frames, the softmax, the CTC alphas.
//
//   max_pooling   torch's max() / min() split the gradient evenly among tied extremes, the clamp passes it where
//                 1e-8 <= v <= 1 (inclusive), masked frames get none:  -(1 / P) / n  resp.  +(1 / Q) / n  on the gated ties
//   ce            softmax(row) - onehot(target)
//   ctc           softmax_t - occupancy_t on the valid frames: alpha (forwards) and beta (backwards) over the extended states in
//                 DOUBLE -- alpha + beta + nll have the magnitude of the row's loss (hundreds), and their rounding is what
//                 limits the occupancies; the reported loss stays the forward's float32 recursion, bit for bit
//
// Every call writes g * upstream / divisor into EVERY element of the gradient (0 beyond the length), a row's values depend on
// that row alone, sums run in a fixed order (no floating-point atomics), `upstream` is a device pointer read by the kernel.
#pragma once
#include "criterion_util.hip.h"

namespace wekws {

constexpr int kCtcGradLdsStates = 1024;     // up to this many extended states the alpha-beta kernel ping-pongs its frames in LDS

__device__ __forceinline__ float crit_clamp01(float v) { return fminf(fmaxf(v, 1e-8f), 1.0f); }

// ------------------------------------------------------------------------------------------------ max pooling
// One wave per (utterance, column).  Pass one: the column's extreme over ALL T frames (a masked frame counts with its fill
// value) and the number of frames that tie with it -- integers, so the merge order plays no role.  Pass two: the writes.
// A NaN in an unmasked frame makes the pooled value NaN; torch then routes the gradient to the NaN frames, where the clamp's
// gate is false: the whole column gets zeros.
__global__ __launch_bounds__(256) void criterion_max_pooling_grad_kernel(const float* __restrict__ scores, int B, int T, int K,
                                                                         const int32_t* __restrict__ target,
                                                                         const int32_t* __restrict__ lengths, int min_duration,
                                                                         const float* __restrict__ upstream, int divisor,
                                                                         float* __restrict__ grad) {
  const int64_t w = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (w >= int64_t(B) * K) return;
  const int lane = threadIdx.x & 63;
  const int b = int(w / K), c = int(w - int64_t(b) * K);
  const int len = lengths ? crit_clampi(lengths[b], 0, T) : T;
  const bool kw = target[b] == c;
  const int t0 = kw && min_duration > 0 ? min_duration : 0;   // m[:min_duration] = True, keyword column only
  const float* p = scores + int64_t(b) * T * K + c;
  float* g = grad + int64_t(b) * T * K + c;
  float ext = 0.0f;
  int n = 0;
  bool nan = false;
  for (int t = lane; t < T; t += kCritWave) {
    const bool masked = t >= len || t < t0;
    const float x = masked ? 0.0f : p[int64_t(t) * K];
    const float u = kw ? x : 1.0f - x;                        // masked: 0 for the keyword, 1 elsewhere
    nan |= u != u;
    const float v = crit_clamp01(u);
    if (n == 0 || (kw ? v > ext : v < ext)) { ext = v; n = 1; }
    else if (v == ext) ++n;
  }
  int anynan = nan ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) {
    const float oe = __shfl_xor(ext, off);
    const int on = __shfl_xor(n, off);
    anynan |= __shfl_xor(anynan, off);
    if (on > 0) {
      if (n == 0 || (kw ? oe > ext : oe < ext)) { ext = oe; n = on; }
      else if (oe == ext) n += on;
    }
  }
  const float mag = (1.0f / ext) / float(n);
  const float val = (kw ? -mag : mag) * (upstream ? upstream[0] : 1.0f) / float(divisor);
  for (int t = lane; t < T; t += kCritWave) {
    const bool masked = t >= len || t < t0;
    bool hit = false;
    if (!masked && !anynan) {
      const float x = p[int64_t(t) * K];
      const float u = kw ? x : 1.0f - x;
      hit = u == ext && u >= 1e-8f && u <= 1.0f;              // inside the gate clamp(u) == u
    }
    g[int64_t(t) * K] = hit ? val : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------ cross entropy
// One wave per row: running max and rescaled sum in one read (as ctc_loss_lp_kernel), then the writes (the row in cache).
__device__ __forceinline__ void crit_wave_max_sum(const float* __restrict__ x, int D, int lane, float& m_out, float& s_out) {
  float m = -INFINITY, s = 0.0f;
  for (int d = lane; d < D; d += kCritWave) {
    const float v = x[d];
    if (v > m) { s = s * crit_scale(m, v) + 1.0f; m = v; }
    else s += v == -INFINITY ? 0.0f : expf(v - m);           // a NaN logit makes s NaN
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(m, off), os = __shfl_xor(s, off);
    const float nm = fmaxf(m, om);
    const bool low = (lane & off) == 0;                       // the lower lane's term first on both lanes of a pair
    const float a = (low ? s : os) * crit_scale(low ? m : om, nm), c = (low ? os : s) * crit_scale(low ? om : m, nm);
    s = a + c;
    m = nm;
  }
  m_out = m;
  s_out = s;
}

__global__ __launch_bounds__(256) void criterion_ce_grad_kernel(const float* __restrict__ logits, int B, int D,
                                                                const int32_t* __restrict__ target,
                                                                const float* __restrict__ upstream, int divisor,
                                                                float* __restrict__ grad) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const float* x = logits + int64_t(b) * D;
  float* g = grad + int64_t(b) * D;
  float m, s;
  crit_wave_max_sum(x, D, lane, m, s);
  const int t = target[b];
  const bool ok = t >= 0 && t < D;
  const float up = upstream ? upstream[0] : 1.0f, div = float(divisor);
  for (int d = lane; d < D; d += kCritWave) {
    const float e = expf(x[d] - m) / s;
    g[d] = ok ? (d == t ? e - 1.0f : e) * up / div : crit_nan();
  }
}

// ------------------------------------------------------------------------------------------------ CTC
// log(e^a + e^b + e^c): the largest term first (its own exponential is 1 and is not computed), the other two through log1p.
__device__ __forceinline__ double crit_lse3d(double a, double b, double c) {
  double t;
  if (b > a) { t = a; a = b; b = t; }
  if (c > a) { t = a; a = c; c = t; }
  if (a == -INFINITY) return -INFINITY;
  return a + log1p(exp(b - a) + exp(c - a));                  // a NaN term survives the sum
}

// Kernel three of the gradient path (after ctc_loss_lp_kernel with its per-frame statistics and the float32 alpha kernel that
// reports the loss): one workgroup per row, states across its lanes (strided beyond the workgroup), one barrier per frame.
//   forwards   alpha_t(s) in double, kept for every frame in ab[b][t][s]
//   nll[b]     -lse(alpha_{len-1}(2S), alpha_{len-1}(2S-1)); NaN for a label outside [1, V), +Inf where no alignment fits
//   backwards  beta_t(s) (with the frame's own emission) ping-ponged; ab[b][t][s] <- alpha + beta - lp + nll, the LOG of the
//              occupancy (-Inf: none) -- its exponential is left to the gradient pass, which has a workgroup per frame for it
//   link[b]    per label: 1 if it is the first occurrence of its class, and the index of the class's next occurrence (-1: none)
// The ping-pong frames live in LDS up to kCtcGradLdsStates states, beyond that in global memory (alpha: ab's own rows; beta: pp).
__global__ void ctc_grad_alpha_beta_kernel(const float* __restrict__ lp, int T, int V, const int32_t* __restrict__ targets,
                                           int Lmax, const int32_t* __restrict__ logit_lengths,
                                           const int32_t* __restrict__ target_lengths, double* ab, double* pp,
                                           double* __restrict__ nll, int32_t* __restrict__ link, int lds_mode) {
  extern __shared__ double cg_lds[];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int S = crit_clampi(target_lengths[b], 0, Lmax);
  const int len = crit_clampi(logit_lengths[b], 0, T);
  const int n = 2 * S + 1, W = 2 * Lmax + 1;
  double* buf0 = lds_mode ? cg_lds : pp + int64_t(b) * 2 * W;
  double* buf1 = buf0 + W;
  int32_t* lab = reinterpret_cast<int32_t*>(cg_lds + (lds_mode ? 2 * W : 0));
  int bad = 0;
  for (int i = tid; i < S; i += nt) {
    const int c = targets[int64_t(b) * Lmax + i];
    lab[i] = c;
    if (c < 1 || c >= V) bad = 1;
  }
  if (__syncthreads_or(bad)) { if (tid == 0) nll[b] = double(crit_nan()); return; }
  for (int i = tid; i < S; i += nt) {
    const int c = lab[i];
    int first = 1, next = -1;
    for (int j = 0; j < i; ++j) if (lab[j] == c) { first = 0; break; }
    for (int j = i + 1; j < S; ++j) if (lab[j] == c) { next = j; break; }
    link[int64_t(b) * 2 * Lmax + i] = first;
    link[int64_t(b) * 2 * Lmax + Lmax + i] = next;
  }
  if (len == 0) { if (tid == 0) nll[b] = S > 0 ? double(INFINITY) : 0.0; return; }
  const float* q = lp + int64_t(b) * T * (Lmax + 1);
  const int stride = Lmax + 1;
  double* A = ab + int64_t(b) * T * W;
  // ---- alpha
  {
    double* cur = lds_mode ? buf0 : A;
    for (int s = tid; s < n; s += nt) {
      const double v = s == 0 ? double(q[0]) : (s == 1 ? double(q[1]) : -INFINITY);
      cur[s] = v;
      if (lds_mode) A[s] = v;
    }
  }
  __syncthreads();
  const double* prev = lds_mode ? buf0 : A;
  const int my = (tid & 1) ? (tid + 1) >> 1 : 0;              // lp column of state tid: its next frame's value is kept in flight
  float nxt = (tid < n && len > 1) ? q[stride + my] : 0.0f;
  for (int t = 1; t < len; ++t) {
    double* cur = lds_mode ? (prev == buf0 ? buf1 : buf0) : A + int64_t(t) * W;
    const float* qt = q + int64_t(t) * stride;
    const float mine = nxt;
    if (tid < n && t + 1 < len) nxt = qt[stride + my];
    for (int s = tid; s < n; s += nt) {
      const int li = s >> 1;
      const double a = prev[s];
      const double bb = s > 0 ? prev[s - 1] : -INFINITY;
      const double c = ((s & 1) && s >= 3 && lab[li] != lab[li - 1]) ? prev[s - 2] : -INFINITY;
      const double v = crit_lse3d(a, bb, c) + double(s == tid ? mine : qt[(s & 1) ? li + 1 : 0]);
      cur[s] = v;
      if (lds_mode) A[int64_t(t) * W + s] = v;
    }
    __syncthreads();
    prev = cur;
  }
  const double ll = crit_lse3d(prev[2 * S], S > 0 ? prev[2 * S - 1] : -INFINITY, -INFINITY);
  if (tid == 0) nll[b] = -ll;
  if (!(ll > -INFINITY && ll < INFINITY)) return;             // no alignment fits (or a NaN logit): the gradient pass writes NaN
  __syncthreads();                                            // everyone has read the last alphas before the frames are reused
  // ---- beta and the occupancies
  double* bprev = buf0;
  {
    const float* qt = q + int64_t(len - 1) * stride;
    double* ar = A + int64_t(len - 1) * W;
    for (int s = tid; s < n; s += nt) {
      const bool end = s == 2 * S || s == 2 * S - 1;
      bprev[s] = end ? double(qt[(s & 1) ? (s >> 1) + 1 : 0]) : -INFINITY;
      ar[s] = end ? ar[s] - ll : -INFINITY;
    }
  }
  __syncthreads();
  double anx = 0.0;                                           // state tid's alpha and lp of the frame before: in flight too
  if (tid < n && len > 1) { nxt = q[int64_t(len - 2) * stride + my]; anx = A[int64_t(len - 2) * W + tid]; }
  for (int t = len - 2; t >= 0; --t) {
    double* bcur = bprev == buf0 ? buf1 : buf0;
    const float* qt = q + int64_t(t) * stride;
    double* ar = A + int64_t(t) * W;
    const float mine = nxt;
    const double amine = anx;
    if (tid < n && t > 0) { nxt = qt[my - stride]; anx = ar[tid - W]; }
    for (int s = tid; s < n; s += nt) {
      const int li = s >> 1;
      const double a = bprev[s];
      const double bb = s + 1 < n ? bprev[s + 1] : -INFINITY;
      const double c = ((s & 1) && s + 2 < n && lab[li + 1] != lab[li]) ? bprev[s + 2] : -INFINITY;
      const double rest = crit_lse3d(a, bb, c);               // beta_t(s) - lp_t(s)
      bcur[s] = rest + double(s == tid ? mine : qt[(s & 1) ? li + 1 : 0]);
      ar[s] = (s == tid ? amine : ar[s]) + rest - ll;         // -Inf where either side is: no +Inf occurs
    }
    __syncthreads();
    bprev = bcur;
  }
}

// One workgroup per frame: g = softmax * scale from the frame's max and log-sum (one read of the logits, one write of the
// gradient; 16-byte accesses in the middle where logits and gradient share their misalignment, scalar at the head and tail --
// V = 2599 is no multiple of 4), then, after a barrier, the classes that occur in the row's labels are written again as
// (softmax - occupancy) * scale by one owner each: thread 0 for the blank (wave 0 adds its S + 1 states: lane k takes states
// k, k + 64, ... in turn, then a butterfly), the thread of a class's FIRST label for that class (its states in ascending order).
__device__ __forceinline__ float crit_softmax_elem(float x, float m, float ls) { return expf((x - m) - ls); }

__device__ __forceinline__ void crit_row_fill(float* __restrict__ g, int V, int tid, int nt, float v) {
  for (int d = tid; d < V; d += nt) g[d] = v;
}

__global__ __launch_bounds__(256) void ctc_grad_kernel(const float* __restrict__ logits, int T, int V,
                                                       const int32_t* __restrict__ targets, int Lmax,
                                                       const int32_t* __restrict__ logit_lengths,
                                                       const int32_t* __restrict__ target_lengths,
                                                       const float* __restrict__ stats, const double* __restrict__ logocc,
                                                       const double* __restrict__ nll, const int32_t* __restrict__ link,
                                                       const float* __restrict__ upstream, int divisor,
                                                       float* __restrict__ grad) {
  const int64_t f = blockIdx.x;                               // frame = b * T + t
  const int tid = threadIdx.x;
  const int b = int(f / T), t = int(f - int64_t(b) * T);
  const float* x = logits + f * V;
  float* g = grad + f * V;
  if (t >= crit_clampi(logit_lengths[b], 0, T)) { crit_row_fill(g, V, tid, 256, 0.0f); return; }
  const double nl = nll[b];
  if (!(nl > -INFINITY && nl < INFINITY)) { crit_row_fill(g, V, tid, 256, crit_nan()); return; }
  const float m = stats[2 * f], ls = stats[2 * f + 1];
  const float scale = (upstream ? upstream[0] : 1.0f) / float(divisor);
  const bool wide = ((reinterpret_cast<uintptr_t>(x) ^ reinterpret_cast<uintptr_t>(g)) & 15) == 0;
  int head = wide ? int(((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) >> 2) : V;
  if (head > V) head = V;
  for (int d = tid; d < head; d += 256) g[d] = crit_softmax_elem(x[d], m, ls) * scale;
  if (wide) {
    const int nv = (V - head) >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x + head);
    float4* g4 = reinterpret_cast<float4*>(g + head);
    for (int i = tid; i < nv; i += 256) {
      const float4 v = x4[i];
      float4 r;
      r.x = crit_softmax_elem(v.x, m, ls) * scale;
      r.y = crit_softmax_elem(v.y, m, ls) * scale;
      r.z = crit_softmax_elem(v.z, m, ls) * scale;
      r.w = crit_softmax_elem(v.w, m, ls) * scale;
      g4[i] = r;
    }
    for (int d = head + 4 * nv + tid; d < V; d += 256) g[d] = crit_softmax_elem(x[d], m, ls) * scale;
  }
  __syncthreads();
  const int S = crit_clampi(target_lengths[b], 0, Lmax);
  const int W = 2 * Lmax + 1;
  const double* o = logocc + f * W;
  if (tid < kCritWave) {
    double sum = 0.0;
    for (int k = tid; k <= S; k += kCritWave) sum += exp(o[2 * k]);
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (tid == 0) g[0] = float(double(crit_softmax_elem(x[0], m, ls)) - sum) * scale;
  }
  const int32_t* first = link + int64_t(b) * 2 * Lmax;
  const int32_t* next = first + Lmax;
  for (int i = tid; i < S; i += 256) {
    if (!first[i]) continue;
    double sum = 0.0;
    for (int k = i; k >= 0; k = next[k]) sum += exp(o[2 * k + 1]);
    const int c = targets[int64_t(b) * Lmax + i];
    g[c] = float(double(crit_softmax_elem(x[c], m, ls)) - sum) * scale;
  }
}

int launch_criterion_max_pooling_grad(const float* scores, int B, int T, int K, const int32_t* target, const int32_t* lengths,
                                      int min_duration, const float* upstream, int divisor, float* grad, hipStream_t stream);
int launch_criterion_ce_grad(const float* logits, int B, int D, const int32_t* target, const float* upstream, int divisor,
                             float* grad, hipStream_t stream);

// The gradient path's workspace, in this order (doubles first: the base is 8-byte aligned).
struct CtcGradWorkspace {
  size_t ab, pp, nll, lp, stats, link, total;                 // byte offsets, and the size
};
inline CtcGradWorkspace ctc_grad_workspace(int B, int T, int Lmax) {
  const size_t b = size_t(B), t = size_t(T), l = size_t(Lmax), w = 2 * l + 1;
  CtcGradWorkspace ws;
  size_t off = 0;
  ws.ab = off;    off += b * t * w * sizeof(double);          // alphas, then occupancies, of every frame
  ws.pp = off;    off += b * 2 * w * sizeof(double);          // the beta ping-pong beyond kCtcGradLdsStates
  ws.nll = off;   off += b * sizeof(double);
  ws.lp = off;    off += b * t * (l + 1) * sizeof(float);     // wekws_hip_ctc_loss's workspace
  ws.stats = off; off += b * t * 2 * sizeof(float);           // the frame's max and log-sum
  ws.link = off;  off += b * 2 * l * sizeof(int32_t);
  ws.total = (off + 15) & ~size_t(15);
  return ws;
}
int launch_ctc_loss_grad(const float* logits, int B, int T, int V, const int32_t* targets, int Lmax, const int32_t* logit_lengths,
                         const int32_t* target_lengths, const float* upstream, int divisor, float* loss_rows, float* loss,
                         float* grad, char* workspace, hipStream_t stream);

}  // namespace wekws
