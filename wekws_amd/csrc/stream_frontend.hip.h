// Streaming front end for many streams at once: the part of KeyWordSpotter.accept_wave (wekws/bin/stream_kws_ctc.py:335-398)
// that runs per PCM chunk -- leftover samples, Kaldi fbank of (leftover + chunk), the remembered feature frames of the context
// expansion, the frame-skip phase -- as two launches per push.  What each row does is decided on the host by stream_fe_plan
// (stream_frontend.h); the kernels are told through one StreamFeRow per row.
//
//   fbank_stream_kernel   frame k of a row is samples [k S, k S + L) of the VIRTUAL concatenation [leftover | chunk]: the int16
//                         leftover buffer of the stream and the row's int16 chunk are read in place, no assembled copy.  The
//                         arithmetic from the DC removal to the logarithm is fbank_frames of fbank.hip.h -- the code
//                         fbank_kernel runs, so a frame equals the one-shot kernel's bit for bit; only the fetch and the store
//                         address differ.  An even leftover keeps every sample pair on one side of the boundary (one 4-byte
//                         load); an odd one makes the chunk side pair-misaligned and takes per-sample select loads.  The wave
//                         that owns a row's frame slot 0 also writes the row's new leftover, samples [nf S, tot) of the same
//                         concatenation (a held row or one without a frame: everything, i.e. an append), into the stream's
//                         OTHER buffer: other waves still read the old one.
//                         Persistent waves walk the (row, frame slot) grid of B x Tv, Tv the call's largest frame count; a slot
//                         past its row's count costs a plan read, no transform.
//                         MFCC mode (template parameter; the log-mel instantiation is the code above and nothing else): the row
//                         sink is the wave's own LDS strip, and the wave that finished the frame applies DCT-II and lifter before
//                         the store -- lane c (and c + 64) runs dct_lifter_kernel's chain for cepstrum c, so a streamed row is
//                         dct_lifter(Fbank(whole))[k] bit for bit.  The (num_bins x num_ceps) matrix is read from GLOBAL memory
//                         (25.6 KB at 80 x 80, consecutive lanes on consecutive words: cache hits); in LDS it would add up to
//                         64 KB per workgroup and cost fbank_stream_kernel<2> its four workgroups per CU.
//   splice_stream_kernel  context and / or skip as a gather over the remembered frames and the fresh ones; writes the caller's
//                         rows and the frames to remember (the stream's other buffer again).  Pure data movement.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fbank.hip.h"
#include "stream_frontend.h"

namespace wekws {

struct StreamFeRow {        // what the kernels know about one row of a push (16 x int32)
  int32_t rem, n, nf, rem_out;
  int32_t lo_old, lo_new;   // sample offsets of the stream's leftover buffers (read / written)
  int32_t fb_base;          // frame slot of the row's first fresh frame in the fbank destination
  int32_t pad_first, fr_in;
  int32_t fr_keep;          // frames to remember (0: held row or no context -- nothing written)
  int32_t rows_out, off;
  int32_t fr_old, fr_new;   // frame offsets of the stream's remembered-frame buffers (read / written)
  int32_t out_base;         // the row's first output row
  int32_t reserved;
};

constexpr int kStreamFeRing = 4;   // plan tables in flight (stream_frontend.hip)

// U (even) steps of dct_lifter_kernel's chain (mfcc.hip.h), from an even row on: s0 takes the even rows, s1 the odd ones, in order.
// x: the log-mel values of the rows (LDS), d: the matrix column of this lane's cepstrum from the same row on (global, stride NC).
template <int U>
__device__ __forceinline__ void dct_rows(const float* x, const float* __restrict__ d, int NC, float& s0, float& s1) {
  float dv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) dv[u] = d[u * NC];
#pragma unroll
  for (int u = 0; u < U; u += 2) {
    s0 = fmaf(x[u], dv[u], s0);
    s1 = fmaf(x[u + 1], dv[u + 1], s1);
  }
}

template <int ROUNDS, bool MFCC>
__global__ __launch_bounds__(64 * kFbankWaves, ROUNDS == 2 ? 4 : 1) void fbank_stream_kernel(
    const FbankParams P, const StreamFeRow* __restrict__ rows, const int16_t* __restrict__ pcm, int B, int nmax, int Tv,
    int16_t* __restrict__ lo, float* __restrict__ dst, int pair_static, const float* __restrict__ dct, int NC) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  float* const strip = lds + wave * kFbankStrip;
  const int FL = P.frame_length;
  const float inv_fl = 1.f / float(FL);
  FbankLane<ROUNDS> K;
  K.init(P, lane);

  // slot g of the launch is frame slot g % Tv of row g / Tv, carried like fbank_kernel's (utterance, frame)
  const int64_t total = int64_t(B) * Tv;
  const int64_t stride = int64_t(gridDim.x) * kFbankWaves;
  const int sq = int(stride / Tv), sr = int(stride - int64_t(sq) * Tv);
  const int64_t f_first = int64_t(blockIdx.x) * kFbankWaves + wave;
  int ub = int(f_first / Tv), ufr = int(f_first - int64_t(ub) * Tv);
  float2 vn[1][4];
  bool live_n = false;
  auto fetch = [&](int b, int k) __attribute__((always_inline)) {
    live_n = false;
    int rem = 0;
    const int16_t* lop = lo;
    const int16_t* chp = lo;
    if (b < B) {
      const StreamFeRow& R = rows[b];
      live_n = k < R.nf;
      rem = R.rem;
      lop = lo + R.lo_old;
      chp = pcm + int64_t(b) * nmax;
    }
    const int base = k * P.frame_shift;
    if (!live_n) {
#pragma unroll
      for (int m = 0; m < 4; ++m) vn[0][m] = make_float2(0.f, 0.f);
    } else if (pair_static && (rem & 1) == 0) {
      // every pair lies on one side of the boundary and is 4-byte aligned there
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int i = 2 * (lane + 64 * m);
        const bool in = i < FL;
        const int j = base + i;
        const int16_t* at = !in ? lo : (j < rem ? lop + j : chp + (j - rem));       // (outside: any valid pair, dropped)
        const short2 q = *reinterpret_cast<const short2*>(at);
        vn[0][m] = in ? make_float2(float(q.x), float(q.y)) : make_float2(0.f, 0.f);
      }
    } else {
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int i = 2 * (lane + 64 * m);
        const int j = base + i;
        float2 v = make_float2(0.f, 0.f);
        if (i < FL) v.x = float(j < rem ? lop[j] : chp[j - rem]);
        if (i + 1 < FL) v.y = float(j + 1 < rem ? lop[j + 1] : chp[j + 1 - rem]);
        vn[0][m] = v;
      }
    }
  };
  fetch(ub, ufr);
  for (int64_t f = f_first; f < total; f += stride) {
    int nb = ub + sq, nfr = ufr + sr;
    if (nfr >= Tv) { nfr -= Tv; ++nb; }
    const bool live = live_n;
    if (ufr == 0) {
      // the row's new leftover: samples [nf S, tot) of the concatenation, into the stream's other buffer
      const StreamFeRow& R = rows[ub];
      const int rem = R.rem, first = R.nf * P.frame_shift, cnt = R.rem_out;
      const int16_t* lop = lo + R.lo_old;
      const int16_t* chp = pcm + int64_t(ub) * nmax;
      int16_t* out = lo + R.lo_new;
      for (int j = lane; j < cnt; j += 64) {
        const int s = first + j;
        out[j] = s < rem ? lop[s] : chp[s - rem];
      }
    }
    if (live) {
      const int64_t slot = int64_t(rows[ub].fb_base) + ufr;
      fbank_frames<ROUNDS, 1>(K, strip, lane, inv_fl, vn, [&]() __attribute__((always_inline)) { fetch(nb, nfr); },
                              [&](int, float*& row) __attribute__((always_inline)) {
                                if constexpr (MFCC) row = strip;             // (the power bins are spent: the strip's head is free)
                                else row = dst + slot * P.num_bins;
                                return true;
                              });
      if constexpr (MFCC) {
        // fbank_frames ends in a wave_sync: the strip holds the frame's num_bins log-mel values.  Cepstrum c is the chain of
        // dct_lifter_kernel (mfcc.hip.h) on the same matrix: s0 over even n, s1 over odd n, s0 + s1.  One cepstrum per pass -- two
        // cepstra in one loop would invite the compiler to pair their chains across the broadcast x (pk_safe.hip.h).
        const int N = P.num_bins;
        float* const out = dst + slot * NC;
        for (int c = lane; c < NC; c += 64) {
          const float* __restrict__ d = dct + c;
          float s0 = 0.f, s1 = 0.f;
          int n = 0;
          // the same chain in blocks of 8 rows whose matrix loads are all issued before the first is used: one load per step,
          // waited for at once, left the wave idle for a cache round trip per pair of rows (16 at a time cost registers: spills
          // in the 128-register instance, a wave per SIMD less in the others)
          for (; n + 8 <= N; n += 8) dct_rows<8>(strip + n, d + n * NC, NC, s0, s1);
          for (; n + 1 < N; n += 2) dct_rows<2>(strip + n, d + n * NC, NC, s0, s1);
          if (n < N) s0 = fmaf(strip[n], d[n * NC], s0);
          out[c] = s0 + s1;
        }
        wave_sync();                                            // every lane has read the row: the strip is free for the next frame
      }
    } else {
      fetch(nb, nfr);
    }
    ub = nb; ufr = nfr;
  }
}

template <typename V>
__global__ __launch_bounds__(256) void splice_stream_kernel(const StreamFeRow* __restrict__ rows, const V* __restrict__ fresh,
                                                            V* __restrict__ frs, V* __restrict__ out, int Fv, int left, int W,
                                                            int skip) {
  const StreamFeRow R = rows[blockIdx.x];
  const int e = int(blockIdx.y) * 256 + threadIdx.x;
  const int n_out = R.rows_out * W * Fv;
  if (e < n_out) {
    const int f = e % Fv;
    int q = e / Fv;
    const int w = q % W;
    const int j = q / W;
    const int p = R.off + j * skip + w;                        // position in [remembered | fresh] or [first x left | fresh]
    const V* src;
    if (R.pad_first) src = fresh + (int64_t(R.fb_base) + (p < left ? 0 : p - left)) * Fv;
    else src = p < R.fr_in ? frs + (int64_t(R.fr_old) + p) * Fv : fresh + (int64_t(R.fb_base) + (p - R.fr_in)) * Fv;
    out[((int64_t(R.out_base) + j) * W + w) * Fv + f] = src[f];
  } else if (e < n_out + R.fr_keep * Fv) {
    const int e2 = e - n_out;
    const int f = e2 % Fv, t = e2 / Fv;
    frs[(int64_t(R.fr_new) + t) * Fv + f] = fresh[(int64_t(R.fb_base) + (R.nf - R.fr_keep + t)) * Fv + f];
  }
}

inline size_t fbank_stream_lds() { return size_t(kFbankWaves * kFbankStrip) * sizeof(float); }

using FbankStreamKernel = void (*)(const FbankParams, const StreamFeRow*, const int16_t*, int, int, int, int16_t*, float*, int,
                                   const float*, int);
inline FbankStreamKernel fbank_stream_instance(int rounds, bool mfcc) {
  if (mfcc) return rounds == 1 ? fbank_stream_kernel<1, true> : rounds == 2 ? fbank_stream_kernel<2, true> : fbank_stream_kernel<3, true>;
  return rounds == 1 ? fbank_stream_kernel<1, false> : rounds == 2 ? fbank_stream_kernel<2, false> : fbank_stream_kernel<3, false>;
}

inline int fbank_stream_resident_groups(const FbankParams& P, bool mfcc) {
  const int rounds = (P.nslots + 63) / 64;
  if (rounds < 1 || rounds > 3) return 0;
  auto kern = fbank_stream_instance(rounds, mfcc);
  int per_cu = 0, dev = 0;
  hipDeviceProp_t prop;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64 * kFbankWaves, fbank_stream_lds()) == hipSuccess &&
      hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && per_cu > 0)
    return per_cu * prop.multiProcessorCount;
  return 256 * 4;
}

// dct: NULL for log-mel rows of P.num_bins floats, else the (num_bins x num_ceps) matrix of launch_dct_lifter_matrix: rows of num_ceps
int launch_fbank_stream(const FbankParams& P, const StreamFeRow* rows, const int16_t* pcm, int B, int nmax, int Tv, int16_t* lo,
                        float* dst, int resident, const float* dct, int num_ceps, hipStream_t stream);
// the matrix of mfcc.hip.h into D (num_bins x num_ceps floats on the device); defined in frame_ops.hip, the unit that emits that header
__attribute__((visibility("hidden"))) int build_dct_lifter_matrix(float* D, int num_bins, int num_ceps, float lifter, hipStream_t stream);
int launch_splice_stream(const StreamFeRow* rows, const float* fresh, float* frs, float* out, int B, int max_items_f, int F,
                         int left, int W, int skip, hipStream_t stream);

}  // namespace wekws
