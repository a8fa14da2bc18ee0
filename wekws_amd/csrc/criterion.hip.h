// The validation criterion on the device: what wekws/model/loss.py::criterion computes after every forward of
// Executor.cv / Executor.test (wekws/utils/executor.py:70-115), forward only.
//
//   max_pooling   loss.py:26-88    per utterance and keyword the pooled posterior (max over the keyword's frames, min of
//                                  1 - p over every other column), -log of it, and the accuracy rule of :74-85
//   ce            loss.py:167-180  F.cross_entropy (mean) + acc_frame (:91-99)
//   ctc           loss.py:135-164  log_softmax + F.ctc_loss(reduction='sum') / B; the alpha recursion only
//   edit distance loss.py:102-132  acc_utterance's Calculator totals, which reduce to the Levenshtein distance between the
//                                  first entry of the final beam (wekws_hip_ctc_kws_search) and the labels
//
// Every result is a pure function of the inputs: a row's values never depend on the batch around it or on the grid, and the
// batch reductions are one fixed-order pass of a single workgroup (criterion_sum_kernel) -- no floating-point atomics.
// The pooled values and the correctness flags involve comparisons only and are bit-exact against the reference; fmaxf /
// fminf drop a NaN where torch's max / min / clamp keep it, so NaNs travel in flags of their own.
#pragma once
#include "criterion_util.hip.h"

namespace wekws {

constexpr int kEditMaxLabels = 3000;        // LDS of the edit-distance kernel: 3 (L + 1) * 4 bytes
constexpr int kEditMaxPathBeam = 64;        // wekws_hip_ctc_kws_create's limit

// Bytes of one beam record as include/wekws_hip.h documents it for wekws_hip_ctc_kws_beam_bytes (the public layout).
inline size_t edit_beam_bytes(int PB, int cap) {
  const size_t pc = size_t(PB) * cap;
  return (8 + 4 * size_t((PB + 1) & ~1) + 16 * size_t(PB) + 8 * pc + 4 * (pc & 1) + 8 * pc + 15) & ~size_t(15);
}

// ------------------------------------------------------------------------------------------------ max pooling
// One wave per utterance, one pass over its (T * K) row.  K <= 64: the wave reads 64 / K whole frames per step (lane = frame
// group * K + column, consecutive lanes consecutive addresses), then column c's groups are folded in group order; K > 64:
// 64 columns at a time, frame by frame.  Only valid frames (t < len) are read: a masked frame contributes a constant.
__global__ __launch_bounds__(256) void criterion_max_pooling_kernel(const float* __restrict__ scores, int B, int T, int K,
                                                                    const int32_t* __restrict__ target,
                                                                    const int32_t* __restrict__ lengths, int min_duration,
                                                                    float* __restrict__ pooled, float* __restrict__ terms,
                                                                    int32_t* __restrict__ correct) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const int len = lengths ? crit_clampi(lengths[b], 0, T) : T;
  const int tgt = target[b];
  const int t_kw = min_duration > 0 ? min_duration : 0;      // m[:min_duration] = True
  const float* row = scores + int64_t(b) * T * K;
  const bool narrow = K <= kCritWave;
  const int G = narrow ? kCritWave / K : 1;
  float best = -INFINITY;                                     // the utterance's max over keywords, lower index on ties
  int best_c = 0x7fffffff;
  bool best_nan = false;
  for (int c0 = 0; c0 < K; c0 += kCritWave) {                 // one trip when K <= 64
    const int c = narrow ? lane % K : c0 + lane;
    const int g = narrow ? lane / K : 0;
    const bool live = narrow ? g < G : c < K;
    float kmax = 1e-8f;                                       // max_t clamp(p or 0, 1e-8, 1) >= 1e-8
    float omin = 1.0f;                                        // min_t clamp(1 - p or 1, 1e-8, 1) <= 1
    float amax = len < T ? 0.0f : -INFINITY;                  // max_t (p, masked frames 0): the accuracy's max_logits
    bool nan_kw = false, nan_v = false;
    if (live) {
      const float* p = row + c;
      for (int t = g; t < len; t += G) {
        const float v = p[int64_t(t) * K];
        const bool isn = v != v;
        nan_v |= isn;
        amax = fmaxf(amax, v);
        omin = fminf(omin, fmaxf(1.0f - v, 1e-8f));
        if (t >= t_kw) { nan_kw |= isn; kmax = fmaxf(kmax, fminf(v, 1.0f)); }
      }
    }
    if (narrow && G > 1) {                                    // fold the frame groups of column c = lane (lanes < K)
      float fk = 1e-8f, fo = 1.0f, fa = len < T ? 0.0f : -INFINITY;
      int fn = 0;
      const int flags = (nan_kw ? 1 : 0) | (nan_v ? 2 : 0);
      for (int gg = 0; gg < G; ++gg) {
        const int src = (lane < K ? lane : 0) + gg * K;
        fk = fmaxf(fk, __shfl(kmax, src));
        fo = fminf(fo, __shfl(omin, src));
        fa = fmaxf(fa, __shfl(amax, src));
        fn |= __shfl(flags, src);
      }
      kmax = fk; omin = fo; amax = fa; nan_kw = fn & 1; nan_v = fn & 2;
    }
    const bool owner = narrow ? lane < K : c < K;
    if (owner) {
      const bool is_kw = c == tgt;
      const float pv = is_kw ? (nan_kw ? crit_nan() : kmax) : (nan_v ? crit_nan() : omin);
      pooled[int64_t(b) * K + c] = pv;
      terms[int64_t(b) * K + c] = -logf(pv);
      if (nan_v) best_nan = true;
      else if (amax > best) { best = amax; best_c = c; }      // a lane's columns ascend: strict > keeps the lowest
    }
  }
  int any_nan = best_nan ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off);
    const int oc = __shfl_xor(best_c, off);
    any_nan |= __shfl_xor(any_nan, off);
    if (ov > best || (ov == best && oc < best_c)) { best = ov; best_c = oc; }
  }
  if (lane == 0) {
    const bool ok = !any_nan && ((best > 0.5f && best_c == tgt) || (best < 0.5f && tgt < 0));
    correct[b] = ok ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------ cross entropy
// One wave per row: max and first arg-max, then sum exp(x - max) (the second pass finds the row in cache).
__global__ __launch_bounds__(256) void criterion_ce_kernel(const float* __restrict__ logits, int B, int D,
                                                           const int32_t* __restrict__ target, float* __restrict__ loss_rows,
                                                           int32_t* __restrict__ pred, int32_t* __restrict__ correct) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & 63;
  const float* x = logits + int64_t(b) * D;
  float m = -INFINITY;
  int mi = 0x7fffffff;
  for (int d = lane; d < D; d += 64) {
    const float v = x[d];
    if (v > m || mi == 0x7fffffff) { m = v; mi = d; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(m, off);
    const int oi = __shfl_xor(mi, off);
    if (oi != 0x7fffffff && (mi == 0x7fffffff || ov > m || (ov == m && oi < mi))) { m = ov; mi = oi; }
  }
  float s = 0.0f;
  for (int d = lane; d < D; d += 64) s += expf(x[d] - m);
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) {
    const int t = target[b];
    const bool ok = t >= 0 && t < D;
    loss_rows[b] = ok ? logf(s) - (x[t] - m) : crit_nan();   // -(log_softmax(x))[t]
    pred[b] = mi;
    correct[b] = ok && s == s && mi == t ? 1 : 0;             // a NaN logit: loss NaN, row incorrect
  }
}

// ------------------------------------------------------------------------------------------------ CTC loss
// Kernel one: per valid frame the row's log-sum-exp in ONE pass over the logits (running max and rescaled sum per lane,
// merged across the wave), then only lp[b][t][0 .. S_b] = log-probability of the blank and of the row's own labels
// (and, if asked for, the frame's posteriors exp(lp) for the beam search of acc_utterance, and the frame's max and
// log-sum for the gradient pass, criterion_grad.hip.h).
__global__ __launch_bounds__(256) void ctc_loss_lp_kernel(const float* __restrict__ logits, int B, int T, int V,
                                                          const int32_t* __restrict__ targets, int Lmax,
                                                          const int32_t* __restrict__ logit_lengths,
                                                          const int32_t* __restrict__ target_lengths, float* __restrict__ lp,
                                                          float* __restrict__ probs, float* __restrict__ stats) {
  const int64_t f = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);       // frame = b * T + t
  if (f >= int64_t(B) * T) return;
  const int lane = threadIdx.x & 63;
  const int b = int(f / T), t = int(f - int64_t(b) * T);
  if (t >= crit_clampi(logit_lengths[b], 0, T)) return;
  const float* x = logits + f * V;
  float m = -INFINITY, s = 0.0f;
  for (int d = lane; d < V; d += 64) {
    const float v = x[d];
    if (v > m) { s = s * crit_scale(m, v) + 1.0f; m = v; }
    else s += v == -INFINITY ? 0.0f : expf(v - m);           // a NaN logit makes s NaN
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(m, off), os = __shfl_xor(s, off);
    const float nm = fmaxf(m, om);
    // both halves in the same order on both lanes of a pair: the lower lane's term first
    const bool low = (lane & off) == 0;
    const float a = (low ? s : os) * crit_scale(low ? m : om, nm), c = (low ? os : s) * crit_scale(low ? om : m, nm);
    s = a + c;
    m = nm;
  }
  const float ls = logf(s);                                  // lp = (x - max) - log(sum): near 0 it keeps the bits that x - (max + log(sum)) loses
  if (stats && lane == 0) { stats[2 * f] = m; stats[2 * f + 1] = ls; }
  const int S = crit_clampi(target_lengths[b], 0, Lmax);
  float* o = lp + f * (Lmax + 1);
  const int32_t* lab = targets + int64_t(b) * Lmax;
  for (int i = lane; i <= S; i += 64) {
    const int c = i == 0 ? 0 : lab[i - 1];
    o[i] = (c >= 0 && c < V) ? (x[c] - m) - ls : crit_nan();
  }
  if (probs) {                                               // the frame's softmax for the decode of acc_utterance (row in cache)
    float* pr = probs + f * V;
    for (int d = lane; d < V; d += 64) pr[d] = expf((x[d] - m) - ls);
  }
}

__device__ __forceinline__ float crit_lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));   // a NaN term survives the sum
}

// Kernel two: the alpha recursion of F.ctc_loss over the 2 S + 1 extended states (blank, l1, blank, ..., lS, blank), states
// across the workgroup's lanes (strided when there are more states than lanes), alpha ping-ponged in LDS, one barrier per
// frame.  The lane's first state has its lp of the next frame in flight while the current one is combined.
__global__ void ctc_loss_alpha_kernel(const float* __restrict__ lp, int T, int V, const int32_t* __restrict__ targets,
                                      int Lmax, const int32_t* __restrict__ logit_lengths,
                                      const int32_t* __restrict__ target_lengths, float* __restrict__ loss_rows) {
  extern __shared__ float crit_lds[];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int S = crit_clampi(target_lengths[b], 0, Lmax);
  const int len = crit_clampi(logit_lengths[b], 0, T);
  const int n = 2 * S + 1, W = 2 * Lmax + 1;
  float* alpha0 = crit_lds;
  float* alpha1 = crit_lds + W;
  int32_t* lab = reinterpret_cast<int32_t*>(crit_lds + 2 * W);
  __shared__ int bad;
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int i = tid; i < S; i += nt) {
    const int c = targets[int64_t(b) * Lmax + i];
    lab[i] = c;
    if (c < 1 || c >= V) bad = 1;
  }
  __syncthreads();
  if (bad) { if (tid == 0) loss_rows[b] = crit_nan(); return; }
  if (len == 0) { if (tid == 0) loss_rows[b] = S > 0 ? INFINITY : 0.0f; return; }
  const float* q = lp + int64_t(b) * T * (Lmax + 1);
  const int stride = Lmax + 1;
  for (int s = tid; s < n; s += nt) alpha0[s] = s == 0 ? q[0] : (s == 1 ? q[1] : -INFINITY);
  __syncthreads();
  const int my = (tid & 1) ? (tid + 1) >> 1 : 0;              // lp column of state tid
  float nxt = (tid < n && len > 1) ? q[stride + my] : 0.0f;
  float* prev = alpha0;
  float* cur = alpha1;
  for (int t = 1; t < len; ++t) {
    const float* qt = q + int64_t(t) * stride;
    const float mine = nxt;
    if (tid < n && t + 1 < len) nxt = qt[stride + my];
    for (int s = tid; s < n; s += nt) {
      const int li = s >> 1;                                  // odd s: label li
      const float a = prev[s];
      const float bb = s > 0 ? prev[s - 1] : -INFINITY;
      const float c = ((s & 1) && s >= 3 && lab[li] != lab[li - 1]) ? prev[s - 2] : -INFINITY;
      const float e = s == tid ? mine : qt[(s & 1) ? li + 1 : 0];
      cur[s] = crit_lse3(a, bb, c) + e;
    }
    __syncthreads();
    float* sw = prev; prev = cur; cur = sw;
  }
  if (tid == 0) {
    const float l1 = prev[2 * S], l2 = S > 0 ? prev[2 * S - 1] : -INFINITY;
    loss_rows[b] = -crit_lse3(l1, l2, -INFINITY);
  }
}

// ------------------------------------------------------------------------------------------------ edit distance
// One wave per utterance: Levenshtein distance between entry 0 of the utterance's beam record (layout:
// include/wekws_hip.h, wekws_hip_ctc_kws_beam_bytes) and its labels, anti-diagonal by anti-diagonal, three diagonals in LDS indexed by the label position.
__global__ __launch_bounds__(64) void ctc_edit_distance_kernel(const char* __restrict__ beams, size_t beam_stride, int PB,
                                                               int cap, const int32_t* __restrict__ targets, int Lmax,
                                                               const int32_t* __restrict__ target_lengths,
                                                               int32_t* __restrict__ dist) {
  extern __shared__ int32_t edit_lds[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const char* rec = beams + size_t(b) * beam_stride;
  const int32_t* head = reinterpret_cast<const int32_t*>(rec);
  const int cnt = head[0];
  const int m = cnt > 0 ? crit_clampi(head[2], 0, cap) : 0;   // len[0]: the best hypothesis' tokens
  const int32_t* hyp = reinterpret_cast<const int32_t*>(rec + 8 + 4 * size_t((PB + 1) & ~1) + 16 * size_t(PB));   // token[0][:]
  const int n = crit_clampi(target_lengths[b], 0, Lmax);
  const int32_t* lab = targets + int64_t(b) * Lmax;
  const int W = Lmax + 1;
  int32_t* d2 = edit_lds;          // diagonal k - 2
  int32_t* d1 = edit_lds + W;      // diagonal k - 1
  int32_t* d0 = edit_lds + 2 * W;  // diagonal k: d[i][k - i], i = label position
  for (int k = 0; k <= n + m; ++k) {
    const int lo = k - m > 0 ? k - m : 0, hi = k < n ? k : n;
    for (int i = lo + lane; i <= hi; i += 64) {
      const int j = k - i;
      int v;
      if (i == 0) v = j;
      else if (j == 0) v = i;
      else {
        const int del = d1[i - 1] + 1, ins = d1[i] + 1, sub = d2[i - 1] + (lab[i - 1] == hyp[j - 1] ? 0 : 1);
        v = del < ins ? del : ins;
        v = sub < v ? sub : v;
      }
      d0[i] = v;
    }
    __syncthreads();
    int32_t* sw = d2; d2 = d1; d1 = d0; d0 = sw;
  }
  if (lane == 0) dist[b] = d1[n];
}

// ------------------------------------------------------------------------------------------------ batch totals
// One workgroup, one fixed order: thread i adds elements i, i + 256, ... in turn, then a binary tree over the 256 partials.
//   out_f[0] = sum(xf[0 .. nf)) / div          (nf = 0: untouched)
//   out_i[0] = sum(a[0 .. ni)),  out_i[1] = sum(w[0 .. ni))  with a clamped to [0, amax]; rows with a <= 0 add nothing to either
__global__ __launch_bounds__(256) void criterion_sum_kernel(const float* __restrict__ xf, int64_t nf, float div,
                                                            float* __restrict__ out_f, const int32_t* __restrict__ a,
                                                            const int32_t* __restrict__ w, int ni, int amax,
                                                            int32_t* __restrict__ out_i) {
  __shared__ float sf[256];
  __shared__ int si[256], sw[256];
  const int tid = threadIdx.x;
  float f = 0.0f;
  for (int64_t i = tid; i < nf; i += 256) f += xf[i];
  int ia = 0, iw = 0;
  for (int i = tid; i < ni; i += 256) {
    const int v = crit_clampi(a[i], 0, amax);
    if (v > 0) { ia += v; if (w) iw += w[i]; }
  }
  sf[tid] = f; si[tid] = ia; sw[tid] = iw;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) { sf[tid] += sf[tid + off]; si[tid] += si[tid + off]; sw[tid] += sw[tid + off]; }
    __syncthreads();
  }
  if (tid == 0) {
    if (nf > 0) out_f[0] = sf[0] / div;
    if (ni > 0) { out_i[0] = si[0]; if (w) out_i[1] = sw[0]; }
  }
}

int launch_criterion_max_pooling(const float* scores, int B, int T, int K, const int32_t* target, const int32_t* lengths,
                                 int min_duration, float* pooled, float* terms, int32_t* correct, float* loss,
                                 int32_t* num_correct, hipStream_t stream);
int launch_criterion_ce(const float* logits, int B, int D, const int32_t* target, float* loss_rows, int32_t* pred,
                        int32_t* correct, float* loss, int32_t* num_correct, hipStream_t stream);
int launch_ctc_edit_distance(const char* beams, size_t beam_stride, int PB, int cap, int B, const int32_t* targets, int Lmax,
                             const int32_t* target_lengths, int32_t* dist, int32_t* totals, hipStream_t stream);

}  // namespace wekws
