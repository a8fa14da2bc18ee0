// On-device CTC prefix beam search and keyword detection: the reference's `ctc_prefix_beam_search`
// (wekws/model/loss.py:206-312), score_ctc's per-utterance detection (wekws/bin/score_ctc.py:183-236) and the post-model
// part of the streaming `KeyWordSpotter` (wekws/bin/stream_kws_ctc.py:106-530), bit-identical to the reference given the
// same float32 posteriors.  The host receives one 32-byte result record per stream and call.
//
// One wave (one 64-thread block) per stream.  Per frame the wave reads the posterior row coalesced, keeps the first-beam
// top-k with the running-best scheme of topk.hip.h (NaN above every number, equal values lower index first), and then
//   - matches prefixes: `prefix_j == prefix_i + (s,)` is the only equality two keys of one frame can have; a 64-bit hash
//     filters the pairs, a token compare confirms them;
//   - one lane walks the touches in the reference's order (token in top-k order, hypothesis in beam order, the same
//     prefix before the extended one) and accumulates each merged entry in that order, in f64 without contraction;
//   - the lanes rank the entries by (score descending, first touch ascending) -- the stable sort of the reference --
//     and write the surviving beam.
// Path nodes are records with identity: a pool of (frame, prob) cells per stream; a hypothesis holds the token array of
// its prefix and the array of its node cells.  The repeated-token update writes through the cell, so every hypothesis
// holding it sees the change, as the reference's shared dicts do.  The pool is compacted (mark, scan, move) when full.
// Beam state lives in device memory per stream; only the per-frame working set is in LDS.  No inter-workgroup
// synchronisation, no spin loops.  A stream's state is only ever touched by its own one-wave workgroup, so the
// workgroup-scope fences of __syncthreads() order the lanes' global writes and reads (the CU's L1 serves the whole
// workgroup); no agent-scope fence (an L2 write-back) is needed per frame.
//
// Keyword sets (ctc_kws_sets.h).  The keywords, the first-beam token set and the threshold belong to a SET; every slot has a
// set id.  The wave reads its slot's id once -- it is wave-uniform --, takes the set's record and from it the mask pointer,
// the keyword block and the threshold.  The tables are written by copies and by the assign kernel only, both ordered
// against the steps by the stream; a table that grew is a new allocation, so a launch keeps reading the one it was given.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctc_kws_sets.h"

#pragma clang fp contract(off)   // the reference evaluates `n_pb + pb * ps + pnb * ps` with one rounding per operation

namespace wekws {

constexpr int kCtcMaxScoreBeam = 8;
constexpr int kCtcMaxPathBeam = 64;
constexpr int kCtcEInval = -1;
constexpr int kCtcECapacity = -5;

// per-stream scalars and the two beam generations (index: parity)
struct CtcSlotHead {
  int32_t nb, parity, pool_used, status, total_frames, last_active_pos;
  double hit_score;
  int32_t len[2][kCtcMaxPathBeam];
  double pb[2][kCtcMaxPathBeam], pnb[2][kCtcMaxPathBeam];
  uint64_t hash[2][kCtcMaxPathBeam];
};

struct CtcResult {   // == wekws_hip_ctc_kws_result
  int32_t status, valid, state, keyword, start, end;
  double score;
};

struct CtcParams {
  int V, K, PB, cap, pool_cap, n_slots;
  size_t slot_bytes;
  char* slots;
  const CtcSetRec* sets;        // one record per set id
  const int32_t* kw_arena;      // the sets' keyword blocks
  const uint32_t* mask_arena;   // the sets' token masks
  const int32_t* slot_set;      // the set id of every slot (offline: of every row); nullptr = set 0 for all
  int n_sets;                   // ids below this have a record
  int min_frames, max_frames, interval_frames, ds;
};

// what a wave takes from its set's record
struct CtcSet {
  const uint32_t* tokset;   // bitmask over the vocabulary, nullptr = no token set
  const int32_t* kw_off;    // n_kw + 1 offsets into kw_tok
  const int32_t* kw_tok;
  int n_kw;
  double threshold;
};
__device__ inline CtcSet ctc_set(const CtcParams& p, int set) {
  const CtcSetRec r = p.sets[set];
  CtcSet o;
  o.tokset = r.mask_word >= 0 ? p.mask_arena + r.mask_word : nullptr;
  o.kw_off = p.kw_arena + r.kw_base;
  o.kw_tok = o.kw_off + r.n_kw + 1;
  o.n_kw = r.n_kw;
  o.threshold = r.threshold;
  return o;
}

struct CtcSlot {
  CtcSlotHead* h;
  int32_t* tok;     // [2][PB][cap]
  int32_t* node;    // [2][PB][cap]
  int32_t* pframe;  // [pool_cap]
  int32_t* mark;    // [pool_cap]
  double* pprob;    // [pool_cap]
};

__host__ __device__ inline size_t ctc_align(size_t v) { return (v + 255) & ~size_t(255); }
__host__ __device__ inline size_t ctc_slot_bytes(int PB, int cap, int pool_cap) {
  return ctc_align(sizeof(CtcSlotHead)) + 2 * ctc_align(size_t(2) * PB * cap * 4) + 2 * ctc_align(size_t(pool_cap) * 4) +
         ctc_align(size_t(pool_cap) * 8);
}
__device__ inline CtcSlot ctc_slot(const CtcParams& p, int s) {
  char* b = p.slots + size_t(s) * p.slot_bytes;
  CtcSlot o;
  o.h = reinterpret_cast<CtcSlotHead*>(b); b += ctc_align(sizeof(CtcSlotHead));
  o.tok = reinterpret_cast<int32_t*>(b); b += ctc_align(size_t(2) * p.PB * p.cap * 4);
  o.node = reinterpret_cast<int32_t*>(b); b += ctc_align(size_t(2) * p.PB * p.cap * 4);
  o.pframe = reinterpret_cast<int32_t*>(b); b += ctc_align(size_t(p.pool_cap) * 4);
  o.mark = reinterpret_cast<int32_t*>(b); b += ctc_align(size_t(p.pool_cap) * 4);
  o.pprob = reinterpret_cast<double*>(b);
  return o;
}

__device__ inline uint64_t ctc_mix(uint64_t h, int s) { return (h ^ uint64_t(uint32_t(s) + 1u)) * 0x100000001b3ull; }
constexpr uint64_t kCtcHash0 = 0xcbf29ce484222325ull;

// a float's rank key for the first beam: NaN above every number; larger key = better
__device__ inline uint32_t ctc_key(float v) {
  const uint32_t u = __float_as_uint(v);
  if (v != v) return 0xffffffffu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// reset(): the initial beam [((), (1.0, 0.0, []))], hit_score 1.0; the pool is empty again
__device__ inline void ctc_reset_head(CtcSlotHead* h) {
  h->nb = 1; h->parity = 0; h->pool_used = 0; h->status = 0; h->hit_score = 1.0;
  h->len[0][0] = 0; h->pb[0][0] = 1.0; h->pnb[0][0] = 0.0; h->hash[0][0] = kCtcHash0;
}

template <int KMAX, int PBMAX>
struct CtcLds {
  static constexpr int EMAX = PBMAX * (KMAX + 1);
  // current beam
  int len[PBMAX], last[PBMAX], head[PBMAX], hframe[PBMAX], dirty[PBMAX];
  double pb[PBMAX], pnb[PBMAX], hprob[PBMAX];
  uint64_t hash[PBMAX];
  // first beam
  int ftok[KMAX], nf;
  double fps[KMAX];
  int16_t match[PBMAX * KMAX], cur_slot[PBMAX], ext_slot[PBMAX * KMAX];
  // merged entries, in first-touch order
  double epb[EMAX], epnb[EMAX];
  uint64_t ehash[EMAX];
  int elen[EMAX], en[EMAX];
  int16_t ebase[EMAX], order[PBMAX];
  int8_t etail[EMAX];
  int nE, flag;
};

// The keyword detection of execute_detection / score_ctc over the beam of parity `par`: hypotheses in beam order,
// the set's keywords in insertion order, first hit wins; is_sublist's range(len(main) - len(check)) quirk included.
// Every lane returns the keyword's index inside the set (-1: none); lane 0 also updates *hit_score, *start and *end.
__device__ inline int ctc_detect(const CtcParams& p, const CtcSet& ks, const CtcSlot& S, int par, int nb, double* hit_score, int* start,
                                 int* end) {
  const int lane = threadIdx.x;
  for (int hy = 0; hy < nb; ++hy) {
    const int L = S.h->len[par][hy];
    const int32_t* tk = S.tok + (size_t(par) * p.PB + hy) * p.cap;
    const int32_t* nd = S.node + (size_t(par) * p.PB + hy) * p.cap;
    for (int k = 0; k < ks.n_kw; ++k) {
      const int o0 = ks.kw_off[k], kl = ks.kw_off[k + 1] - o0;
      if (L < kl) continue;
      const int n_off = (L == kl) ? 1 : L - kl;
      int off = -1;
      for (int b0 = 0; b0 < n_off && off < 0; b0 += 64) {
        const int i = b0 + lane;
        bool ok = i < n_off;
        for (int m = 0; ok && m < kl; ++m) ok = tk[i + m] == ks.kw_tok[o0 + m];
        const uint64_t bal = __ballot(ok);
        if (bal) off = b0 + __ffsll((unsigned long long)bal) - 1;
      }
      if (off >= 0) {
        if (lane == 0) {
          double hs = *hit_score;
          for (int m = 0; m < kl; ++m) hs = hs * S.pprob[nd[off + m]];
          *hit_score = __dsqrt_rn(hs);
          *start = S.pframe[nd[off]];
          *end = S.pframe[nd[off + kl - 1]];
        }
        return k;
      }
    }
  }
  return -1;
}

// Pool compaction: the cells reachable from the beam of parity `par` move to the front, in order; node arrays remapped.
__device__ inline void ctc_compact(const CtcParams& p, const CtcSlot& S, int par, int nb) {
  const int lane = threadIdx.x;
  const int used = S.h->pool_used;
  for (int c = lane; c < used; c += 64) S.mark[c] = 0;
  __syncthreads();
  for (int e = 0; e < nb; ++e) {
    const int L = S.h->len[par][e];
    const int32_t* nd = S.node + (size_t(par) * p.PB + e) * p.cap;
    for (int i = lane; i < L; i += 64) S.mark[nd[i]] = 1;
  }
  __syncthreads();
  int run = 0;
  for (int b0 = 0; b0 < used; b0 += 64) {
    const int c = b0 + lane;
    const bool live = c < used && S.mark[c] != 0;
    const uint64_t bal = __ballot(live);
    const int dst = run + __popcll(bal & ((1ull << lane) - 1ull));
    int fr = 0;
    double pr = 0.0;
    if (live) { fr = S.pframe[c]; pr = S.pprob[c]; }
    __syncthreads();
    if (live) { S.pframe[dst] = fr; S.pprob[dst] = pr; S.mark[c] = dst; }
    run += __popcll(bal);
  }
  __syncthreads();
  for (int e = 0; e < nb; ++e) {
    const int L = S.h->len[par][e];
    int32_t* nd = S.node + (size_t(par) * p.PB + e) * p.cap;
    for (int i = lane; i < L; i += 64) nd[i] = S.mark[nd[i]];
  }
  if (lane == 0) S.h->pool_used = run;
  __syncthreads();
}

// One frame of the search on the slot's current beam; `tokset`: the first-beam token set of the slot's keyword set, or
// nullptr.  Returns 0, or a status (the beam is then left as it was).
template <int KMAX, int PBMAX>
__device__ int ctc_frame(const CtcParams& p, const uint32_t* tokset, const CtcSlot& S, CtcLds<KMAX, PBMAX>& L, const float* row, int t) {
  const int lane = threadIdx.x;
  const int K = p.K, PB = p.PB;
  // ---- first beam: the lane's k best over a strided slice, then k rounds of a wave-wide arg-max
  uint32_t bk[KMAX];
  int bi[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) { bk[j] = 0; bi[j] = 0x7fffffff; }
  bool inf = false;
  auto take = [&](float v, int k) __attribute__((always_inline)) {
    inf |= __builtin_isinf(v);
    const uint32_t key = ctc_key(v);
    if (key > bk[KMAX - 1]) {   // indices ascend within a lane: strict > keeps the lower index first
      bk[KMAX - 1] = key; bi[KMAX - 1] = k;
#pragma unroll
      for (int j = KMAX - 1; j > 0; --j)
        if (bk[j] > bk[j - 1]) {
          const uint32_t a = bk[j]; bk[j] = bk[j - 1]; bk[j - 1] = a;
          const int b = bi[j]; bi[j] = bi[j - 1]; bi[j - 1] = b;
        }
    }
  };
  struct __attribute__((packed, aligned(4))) V4 { float v[4]; };
  const int V = p.V, V4n = V & ~3;
  for (int k = lane * 4; k < V4n; k += 256) {
    const V4 q = *reinterpret_cast<const V4*>(row + k);
#pragma unroll
    for (int j = 0; j < 4; ++j) take(q.v[j], k + j);
  }
  if (V4n + lane < V) take(row[V4n + lane], V4n + lane);
  if (__ballot(inf)) return kCtcEInval;
  int nf = 0;
  for (int r = 0; r < K; ++r) {
    uint32_t v = bk[0];
    int i = bi[0];
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t ov = __shfl_xor(v, off);
      const int oi = __shfl_xor(i, off);
      if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    if (bi[0] == i) {
#pragma unroll
      for (int j = 0; j < KMAX - 1; ++j) { bk[j] = bk[j + 1]; bi[j] = bi[j + 1]; }
      bk[KMAX - 1] = 0; bi[KMAX - 1] = 0x7fffffff;
    }
    if (i != 0x7fffffff) {
      const float f = row[i];
      const double ps = double(f);
      const bool in_set = !tokset || ((tokset[i >> 5] >> (i & 31)) & 1u);
      if (ps > 0.05 && in_set) {     // NaN fails the comparison: dropped after taking its place
        if (lane == 0) { L.ftok[nf] = i; L.fps[nf] = ps; }
        ++nf;
      }
    }
  }
  if (nf == 0) return 0;   // no token survives: the beam stays as it is
  // ---- current beam into LDS
  CtcSlotHead* H = S.h;
  const int par = H->parity, nb = H->nb;
  for (int j = lane; j < nb; j += 64) {
    const int len = H->len[par][j];
    L.len[j] = len; L.pb[j] = H->pb[par][j]; L.pnb[j] = H->pnb[par][j]; L.hash[j] = H->hash[par][j];
    L.dirty[j] = 0;
    if (len > 0) {
      const int c = S.node[(size_t(par) * PB + j) * p.cap + len - 1];
      L.last[j] = S.tok[(size_t(par) * PB + j) * p.cap + len - 1];
      L.head[j] = c; L.hframe[j] = S.pframe[c]; L.hprob[j] = S.pprob[c];
    } else {
      L.last[j] = -1; L.head[j] = -1;
    }
    L.cur_slot[j] = -1;
  }
  for (int q = lane; q < nb * KMAX; q += 64) { L.match[q] = -1; L.ext_slot[q] = -1; }
  __syncthreads();
  // ---- prefix matches: prefix_j == prefix_i + (s,)  <=>  len, last token, hash agree and the tokens compare equal
  for (int q = lane; q < nb * nb; q += 64) {
    const int i = q / nb, j = q % nb;
    if (L.len[j] != L.len[i] + 1 || L.hash[j] != ctc_mix(L.hash[i], L.last[j])) continue;
    const int32_t* ti = S.tok + (size_t(par) * PB + i) * p.cap;
    const int32_t* tj = S.tok + (size_t(par) * PB + j) * p.cap;
    bool eq = true;
    for (int m = 0; eq && m < L.len[i]; ++m) eq = ti[m] == tj[m];
    if (!eq) continue;
    for (int si = 0; si < nf; ++si)
      if (L.ftok[si] == L.last[j]) L.match[i * KMAX + si] = int16_t(j);
  }
  __syncthreads();
  // ---- the touches, in the reference's order (one lane)
  if (lane == 0) {
    int nE = 0;
    auto make = [&](int len, uint64_t hash) {
      const int e = nE++;
      L.epb[e] = 0.0; L.epnb[e] = 0.0; L.elen[e] = len; L.ehash[e] = hash; L.ebase[e] = -1; L.en[e] = 0; L.etail[e] = -1;
      return e;
    };
    auto cur_entry = [&](int j, bool& fresh) {
      int e = L.cur_slot[j];
      fresh = e < 0;
      if (fresh) { e = make(L.len[j], L.hash[j]); L.cur_slot[j] = int16_t(e); }
      return e;
    };
    auto ext_entry = [&](int i, int si, bool& fresh) {
      const int j = L.match[i * KMAX + si];
      if (j >= 0) return cur_entry(j, fresh);
      int e = L.ext_slot[i * KMAX + si];
      fresh = e < 0;
      if (fresh) { e = make(L.len[i] + 1, ctc_mix(L.hash[i], L.ftok[si])); L.ext_slot[i * KMAX + si] = int16_t(e); }
      return e;
    };
    for (int si = 0; si < nf; ++si) {
      const int s = L.ftok[si];
      const double ps = L.fps[si];
      for (int j = 0; j < nb; ++j) {
        const double pb = L.pb[j], pnb = L.pnb[j];
        bool fresh;
        if (s == 0) {
          const int e = cur_entry(j, fresh);
          L.epb[e] = L.epb[e] + pb * ps + pnb * ps;
          L.ebase[e] = int16_t(j); L.en[e] = L.len[j]; L.etail[e] = -1;
        } else if (s == L.last[j]) {
          if (!(fabs(pnb) <= 1e-6)) {
            const int e = cur_entry(j, fresh);
            L.epnb[e] = L.epnb[e] + pnb * ps;
            L.ebase[e] = int16_t(j); L.en[e] = L.len[j]; L.etail[e] = -1;
            if (ps > L.hprob[j]) { L.hprob[j] = ps; L.hframe[j] = t; L.dirty[j] = 1; }
          }
          if (!(fabs(pb) <= 1e-6)) {
            const int e = ext_entry(j, si, fresh);
            L.epnb[e] = L.epnb[e] + pb * ps;
            L.ebase[e] = int16_t(j); L.en[e] = L.len[j]; L.etail[e] = int8_t(si);
          }
        } else {
          const int e = ext_entry(j, si, fresh);
          if (!fresh) {
            const int tl = L.etail[e];
            const double lastp = tl >= 0 ? L.fps[tl] : L.hprob[L.ebase[e]];
            if (ps > lastp) {                        // pop the entry's last node, append a new one
              if (tl < 0) L.en[e] = L.en[e] - 1;
              L.etail[e] = int8_t(si);
            }
          } else {
            L.ebase[e] = int16_t(j); L.en[e] = L.len[j]; L.etail[e] = int8_t(si);
          }
          L.epnb[e] = L.epnb[e] + pb * ps + pnb * ps;
        }
      }
    }
    L.nE = nE;
  }
  __syncthreads();
  // ---- stable descending sort by pb + pnb; the first PB survive
  const int nE = L.nE;
  const int ns = nE < PB ? nE : PB;
  for (int e = lane; e < nE; e += 64) {
    const double se = L.epb[e] + L.epnb[e];
    int rank = 0;
    for (int f = 0; f < nE; ++f) {
      const double sf = L.epb[f] + L.epnb[f];
      rank += (sf > se) || (sf == se && f < e);
    }
    if (rank < ns) L.order[rank] = int16_t(e);
  }
  __syncthreads();
  // ---- a prefix beyond the capacity fails the stream (never truncated)
  bool over = false;
  for (int r = lane; r < ns; r += 64) {
    const int e = L.order[r];
    over |= L.en[e] + (L.etail[e] >= 0) > p.cap;
  }
  if (__ballot(over)) return kCtcECapacity;
  // ---- node writes through the shared cells
  for (int j = lane; j < nb; j += 64)
    if (L.dirty[j]) { S.pframe[L.head[j]] = L.hframe[j]; S.pprob[L.head[j]] = L.hprob[j]; }
  __syncthreads();
  if (H->pool_used + ns > p.pool_cap) ctc_compact(p, S, par, nb);
  // ---- the new beam into the other generation
  const int np = par ^ 1;
  const int base_cell = H->pool_used;
  const bool tail = lane < ns && L.etail[L.order[lane]] >= 0;
  const uint64_t tb = __ballot(tail);
  if (tail) {
    const int e = L.order[lane];
    const int c = base_cell + __popcll(tb & ((1ull << lane) - 1ull));
    S.pframe[c] = t; S.pprob[c] = L.fps[L.etail[e]];
    const size_t o = (size_t(np) * PB + lane) * p.cap + L.en[e];
    S.tok[o] = L.ftok[L.etail[e]];
    S.node[o] = c;
  }
  for (int r = 0; r < ns; ++r) {
    const int e = L.order[r];
    const int b = L.ebase[e], n = L.en[e];
    const int32_t* st = S.tok + (size_t(par) * PB + b) * p.cap;
    const int32_t* sn = S.node + (size_t(par) * PB + b) * p.cap;
    int32_t* dt = S.tok + (size_t(np) * PB + r) * p.cap;
    int32_t* dn = S.node + (size_t(np) * PB + r) * p.cap;
    for (int i = lane; i < n; i += 64) { dt[i] = st[i]; dn[i] = sn[i]; }
  }
  if (lane < ns) {
    const int e = L.order[lane];
    H->len[np][lane] = L.elen[e]; H->pb[np][lane] = L.epb[e]; H->pnb[np][lane] = L.epnb[e]; H->hash[np][lane] = L.ehash[e];
  }
  __syncthreads();
  if (lane == 0) { H->pool_used = base_cell + __popcll(tb); H->nb = ns; H->parity = np; }
  __syncthreads();
  return 0;
}

// The beam of a slot, for the host: [int32 count, pad][int32 len[PBe]][f64 pb[PB]][f64 pnb[PB]][int32 tok[PB][cap]]
// [int32 frame[PB][cap] (+1 pad if PB * cap is odd)][f64 prob[PB][cap]]; PBe = PB rounded up to even.
__host__ __device__ inline size_t ctc_beam_bytes(int PB, int cap) {
  const size_t pc = size_t(PB) * cap;
  return (8 + 4 * size_t((PB + 1) & ~1) + 16 * size_t(PB) + 8 * pc + 4 * (pc & 1) + 8 * pc + 15) & ~size_t(15);
}
__device__ inline void ctc_write_beam(const CtcParams& p, const CtcSlot& S, char* o) {
  const int lane = threadIdx.x;
  int32_t* cnt = reinterpret_cast<int32_t*>(o);
  int32_t* lens = cnt + 2;
  double* opb = reinterpret_cast<double*>(o + 8 + 4 * ((p.PB + 1) & ~1));
  double* opnb = opb + p.PB;
  const size_t pc = size_t(p.PB) * p.cap;
  int32_t* otok = reinterpret_cast<int32_t*>(opnb + p.PB);
  int32_t* ofr = otok + pc;
  double* opr = reinterpret_cast<double*>(ofr + pc + (pc & 1));
  const CtcSlotHead* H = S.h;
  const int par = H->parity, nb = H->nb;
  if (lane == 0) cnt[0] = nb;
  for (int e = 0; e < nb; ++e) {
    const int len = H->len[par][e];
    if (lane == 0) { lens[e] = len; opb[e] = H->pb[par][e]; opnb[e] = H->pnb[par][e]; }
    for (int i = lane; i < len; i += 64) {
      const size_t src = (size_t(par) * p.PB + e) * p.cap + i, dst = size_t(e) * p.cap + i;
      const int c = S.node[src];
      otok[dst] = S.tok[src]; ofr[dst] = S.pframe[c]; opr[dst] = S.pprob[c];
    }
  }
}

__global__ __launch_bounds__(64) void ctc_kws_read_beam_kernel(CtcParams p, int id, char* out) {
  ctc_write_beam(p, ctc_slot(p, id), out);
}

// mode 0 (streaming step): row b continues stream ids[b] with counts[b] frames.  mode 1 (offline search): row b is a
// fresh utterance of counts[b] frames in slot b; `beams` (optional) receives its final beam.  Either way the slot's
// keyword set is p.slot_set[slot].
template <int KMAX, int PBMAX>
__global__ __launch_bounds__(64) void ctc_kws_kernel(CtcParams p, int mode, const float* __restrict__ probs, int T,
                                                     const int32_t* __restrict__ ids, const int32_t* __restrict__ counts,
                                                     CtcResult* __restrict__ results, char* beams, size_t beam_stride) {
  __shared__ CtcLds<KMAX, PBMAX> L;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = counts ? counts[b] : T;
  CtcResult res{0, 1, 0, -1, 0, 0, 1.0};
  const int sid = mode == 0 ? ids[b] : b;
  if (sid < 0 || sid >= p.n_slots || n < 0 || n > T) {
    if (lane == 0) { res.status = kCtcEInval; results[b] = res; }
    return;
  }
  const int set = p.slot_set ? __builtin_amdgcn_readfirstlane(p.slot_set[sid]) : 0;
  if (set < 0 || set >= p.n_sets) {
    if (lane == 0) { res.status = kCtcEInval; results[b] = res; }
    return;
  }
  const CtcSet ks = ctc_set(p, set);
  const CtcSlot S = ctc_slot(p, sid);
  CtcSlotHead* H = S.h;
  if (mode == 1) {
    if (lane == 0) { ctc_reset_head(H); H->total_frames = 0; H->last_active_pos = -1; }
    __syncthreads();
  }
  if (mode == 0 && n == 0) {           // the reference's `{}`: nothing changes
    if (lane == 0) { res.valid = 0; res.status = H->status; res.score = H->hit_score; results[b] = res; }
    return;
  }
  if (H->status) {
    if (lane == 0) { res.status = H->status; res.score = H->hit_score; results[b] = res; }
    return;
  }
  const float* x = probs + size_t(b) * T * p.V;
  if (mode == 1) {
    for (int t = 0; t < n; ++t) {
      const int st = ctc_frame<KMAX, PBMAX>(p, ks.tokset, S, L, x + size_t(t) * p.V, t);
      if (st) { if (lane == 0) H->status = st; break; }
    }
    __syncthreads();
    double hs = 1.0;
    int start = 0, end = 0;
    const int kw = H->status ? -1 : ctc_detect(p, ks, S, H->parity, H->nb, &hs, &start, &end);
    if (lane == 0) {
      res.status = H->status; res.state = kw >= 0; res.keyword = kw; res.start = start; res.end = end; res.score = hs;
      results[b] = res;
    }
    if (beams && !H->status) ctc_write_beam(p, S, beams + size_t(b) * beam_stride);
    return;
  }
  // ---- streaming: KeyWordSpotter.forward after the model
  int st = 0;
  for (int t = 0; t < n; ++t) {
    const int at = t * p.ds + H->total_frames;
    st = ctc_frame<KMAX, PBMAX>(p, ks.tokset, S, L, x + size_t(t) * p.V, at);
    if (st) break;
    double hs = H->hit_score;
    int start = 0, end = 0;
    const int kw = ctc_detect(p, ks, S, H->parity, H->nb, &hs, &start, &end);
    int act = 0;
    if (lane == 0) {
      if (kw >= 0) {
        H->hit_score = hs;
        const int dur = end - start;
        if (hs >= ks.threshold && p.min_frames <= dur && dur <= p.max_frames &&
            (H->last_active_pos == -1 || end - H->last_active_pos >= p.interval_frames)) {
          act = 1;
          H->last_active_pos = end;
        }
      }
      res.state = act; res.keyword = kw; res.start = start; res.end = end; res.score = H->hit_score;
      if (act) ctc_reset_head(H);
      L.flag = act;
    }
    __syncthreads();
    if (L.flag) break;
  }
  if (lane == 0) {
    if (st) {
      H->status = st;
      res = CtcResult{st, 1, 0, -1, 0, 0, H->hit_score};
    } else {
      H->total_frames += n * p.ds;
      // aging: the first node of the best hypothesis started more than max_frames ago
      const int par = H->parity;
      if (H->nb > 0 && H->len[par][0] > 0) {
        const int kms = S.pframe[S.node[size_t(par) * p.PB * p.cap]];
        if (H->total_frames - kms > p.max_frames) ctc_reset_head(H);
      }
    }
    results[b] = res;
  }
}

__global__ void ctc_kws_reset_kernel(CtcParams p, const int32_t* ids, int n, int all) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = ids[i];
  if (s < 0 || s >= p.n_slots) return;
  CtcSlotHead* h = ctc_slot(p, s).h;
  ctc_reset_head(h);
  if (all) { h->total_frames = 0; h->last_active_pos = -1; }
}

// streams ids[i] take the keyword sets sets[i] and start over as by reset_all; the host has checked ids and sets
__global__ void ctc_kws_assign_kernel(CtcParams p, int32_t* slot_set, const int32_t* ids, const int32_t* sets, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = ids[i];
  if (s < 0 || s >= p.n_slots) return;
  slot_set[s] = sets[i];
  CtcSlotHead* h = ctc_slot(p, s).h;
  ctc_reset_head(h);
  h->total_frames = 0; h->last_active_pos = -1;
}

__global__ void ctc_kws_init_kernel(CtcParams p) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= p.n_slots) return;
  CtcSlotHead* h = ctc_slot(p, s).h;
  ctc_reset_head(h);
  h->total_frames = 0; h->last_active_pos = -1;
}

// host launchers (ctc_kws.hip)
int launch_ctc_kws(const CtcParams& p, int mode, const float* probs, int B, int T, const int32_t* ids,
                   const int32_t* counts, CtcResult* results, char* beams, size_t beam_stride, hipStream_t stream);
int launch_ctc_kws_reset(const CtcParams& p, const int32_t* ids, int n, int all, hipStream_t stream);
int launch_ctc_kws_assign(const CtcParams& p, int32_t* slot_set, const int32_t* ids, const int32_t* sets, int n, hipStream_t stream);
int launch_ctc_kws_init(const CtcParams& p, hipStream_t stream);
int launch_ctc_kws_read_beam(const CtcParams& p, int id, char* out, hipStream_t stream);

}  // namespace wekws
