// The resampler on the device: torchaudio's Resample (resample_plan.h states the definition) as a polyphase FIR over the live
// taps of every phase, for whole utterances (one-shot) and for chunks of many streams (streaming), by ONE kernel.  What a row
// is -- an utterance from its first sample, or a stream's [history | chunk] continued at its next output -- is decided on
// the host and told through one ResampleRow; the arithmetic of an output sample is resample_sample for both, the live taps of
// the output's phase in ascending m with fmaf from 0, so a stream's sample equals the one-shot sample bit for bit.
//
//   workgroup   256 lanes, one output per lane, 256 consecutive outputs of a row per tile; persistent over the (row, tile)
//               grid, so the tap table is loaded once per workgroup.
//   LDS         the live part of the tap table, (n, stride) floats with an odd stride (neighbouring lanes hold neighbouring
//               phases: rows stride apart fall on different banks), the live range of every phase, and the tile's input in
//               its source type (int16 / float) -- every sample under the FULL K-tap windows of the tile's outputs, staged
//               with 16-byte loads wherever 16 source bytes lie inside the row's chunk (the tile's start is moved down to the
//               source's alignment), sample by sample across the history / chunk seam and the row's ends (zeros outside).
//   non-finite  (float input) the reference convolves all K taps, the zeros included, and 0 NaN = 0 Inf = NaN.  Staging sees
//               every sample under the full windows; a tile that holds an all-ones exponent recomputes its outputs over the
//               K taps of the full table in global memory, in plain IEEE f32.  Finite input never takes that path.
//               The scan is over the whole staged tile: up to 7 samples of alignment slack in front, and behind the windows of
//               the tile's outputs whatever the tile's capacity (sized for the most j-blocks 256 outputs can touch) still holds.
//               A NaN / Inf just outside the windows therefore sends the tile down the K-tap path without need.  Its outputs
//               are then the same sums with terms of (+-0) x added: within the bar, equal as numbers, but a sum of -0 can come
//               out as +0 -- that path is not bit-identical to the live-tap path on such a tile.
//   history     the workgroup of a row's tile 0 writes the samples the stream keeps into the stream's OTHER buffer: the
//               other tiles still read the old one.
//   int16 out   rint (half to even), then saturation to [-32768, 32767]; NaN gives 0.
//   chunk       what a row's chunk is in memory is apart from the sample type In of the history and of LDS: ResampleChunk<In>,
//               samples of In themselves, or ResampleWireChunk, the bytes of a wire encoding (wire.h) decoded to int16 where they
//               are fetched -- in the staging loop and in the history write-back, nowhere else.  The encoding is the row's
//               (ResampleRow::wire), so it is uniform over the workgroup: the branches on it are scalar.  A group of 4 samples is
//               one aligned load of a dword (single-byte encodings), of 8 bytes (int16) or of 16 bytes (float32), decoded in
//               registers and stored to LDS as 8 bytes of int16; the row's ragged head and tail go sample by sample, like the
//               seam.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <type_traits>
#include <vector>

#include "resample_plan.h"
#include "wire.h"

namespace wekws {

constexpr int kResampleRing = 4;              // row tables in flight (resample_bank.hip: take_slot)

struct ResampleRow {        // what the kernel knows about one row (12 x int32); positions are relative to the row's origin:
                            // sample 0 of an utterance, the first kept sample of a stream
  int32_t i0;               // phase of the row's first output
  int32_t base_rel;         // position of tap 0 of that output's block: j0 o - width - origin
  int32_t cnt;              // outputs to compute
  int32_t h;                // history samples: positions [0, h) are the stream's buffer, [h, hi_valid) the chunk
  int32_t hi_valid;         // end of the samples there are (zeros beyond, and before 0)
  int32_t hist_old, hist_new;   // sample offsets of the stream's history buffers (read / written)
  int32_t keep_from, keep_cnt;  // positions [keep_from, keep_from + keep_cnt) become the new history
  int32_t member, row;          // rate bank alone (resample_bank.hip.h): the row's plan, and its place in x and y
  int32_t wire;                 // wire calls of the rate bank alone: the encoding of the row's chunk (enum wekws_hip_wire); else 0
};

struct ResampleParams {
  int32_t o, n, K, width;
  int32_t stride;           // floats per row of the live table (odd)
  int32_t tile_cap;         // samples of the input tile (a multiple of kResampleVec)
  int32_t tile_off;         // its byte offset in LDS (a multiple of 16)
  int32_t reserved;
  const float* live;        // (n, stride): taps first_i .. last_i of phase i, then zeros
  const int32_t* first;     // (n)
  const int32_t* count;     // (n) live taps of every phase
  const float* full;        // (n, K)
};

// One output sample: the live taps of its phase, ascending, fmaf from 0.  taps: the phase's row of the live table; x: the sample
// under the first live tap.
template <typename In>
__device__ __forceinline__ float resample_sample(const float* taps, int cnt, const In* x) {
  float acc = 0.f;
  for (int m = 0; m < cnt; ++m) acc = fmaf(taps[m], float(x[m]), acc);
  return acc;
}

__device__ __forceinline__ int resample_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// ---- a row's chunk.  Sample: the type it delivers (the history's and the LDS tile's); kGroup: samples of one staged group, at most
// kResampleVec (the slack the tile's capacity holds); at(k): sample k; slack(k): how many samples position k lies behind the alignment stage() loads at; stage(dst, k):
// the group at an aligned position k, whole inside the chunk, to LDS -- returns whether it holds a non-finite value (float alone).
template <typename In>
struct ResampleChunk {                       // samples of the kernel's own type
  typedef In Sample;
  typedef In Src;
  static constexpr int kGroup = 16 / int(sizeof(In));
  static constexpr bool kPlain = true;       // a sample is a plain load from p
  const In* p;
  __device__ __forceinline__ ResampleChunk(const In* row, const ResampleRow&) : p(row) {}
  __device__ __forceinline__ In at(int k) const { return p[k]; }
  __device__ __forceinline__ int slack(int k) const {
    const int64_t src = int64_t(reinterpret_cast<uintptr_t>(p) / sizeof(In)) + k;
    return int(((src % kGroup) + kGroup) % kGroup);           // down to a 16-byte boundary of the chunk
  }
  __device__ __forceinline__ int stage(In* dst, int k) const {
    const uint4 v = *reinterpret_cast<const uint4*>(p + k);
    *reinterpret_cast<uint4*>(dst) = v;
    if constexpr (std::is_same<In, float>::value)
      return resample_nonfinite(__uint_as_float(v.x)) | resample_nonfinite(__uint_as_float(v.y)) |
             resample_nonfinite(__uint_as_float(v.z)) | resample_nonfinite(__uint_as_float(v.w));
    else
      return 0;
  }
};

struct ResampleWireChunk {                   // bytes of the row's wire encoding (wire.h): p is 4-byte aligned (the plan's check)
  typedef int16_t Sample;
  typedef uint8_t Src;
  // Four samples per lane and group: the decode is VALU work of the staging lanes alone, and a tile's input is few groups (an 8 kHz
  // tile reads ~160 samples), so narrower groups put more lanes to it -- one dword of single bytes, 8 bytes of int16, 16 of float32.
  static constexpr int kGroup = 4;
  static constexpr bool kPlain = false;
  const uint8_t* p;
  int enc, bytes;                            // uniform over the workgroup (the row's): every branch on them is scalar
  __device__ __forceinline__ ResampleWireChunk(const uint8_t* row, const ResampleRow& R)
      : p(row), enc(R.wire), bytes(wire_sample_bytes(R.wire)) {}
  __device__ __forceinline__ int16_t at(int k) const {
    if (enc == WEKWS_HIP_WIRE_MULAW) return int16_t(wire_mulaw(p[k]));
    if (enc == WEKWS_HIP_WIRE_ALAW) return int16_t(wire_alaw(p[k]));
    if (enc == WEKWS_HIP_WIRE_U8) return int16_t(wire_u8(p[k]));
    if (enc == WEKWS_HIP_WIRE_F32) return int16_t(wire_f32(reinterpret_cast<const float*>(p)[k]));
    return reinterpret_cast<const int16_t*>(p)[k];
  }
  // a group is 4, 8 or 16 source bytes, loaded at its own size's alignment: at most 3 samples of slack
  // (sizes and alignments are powers of two: a mask and a shift, where a division by a run-time value would be a long routine)
  __device__ __forceinline__ int slack(int k) const {
    const uint64_t addr = uint64_t(reinterpret_cast<uintptr_t>(p)) + uint64_t(int64_t(k) * bytes);
    return int(uint32_t(addr) & uint32_t(kGroup * bytes - 1)) >> (bytes >> 1);
  }
  static __device__ __forceinline__ uint2 pack(int v0, int v1, int v2, int v3) {
    return make_uint2((uint32_t(v0) & 0xffffu) | (uint32_t(v1) << 16), (uint32_t(v2) & 0xffffu) | (uint32_t(v3) << 16));
  }
  __device__ __forceinline__ int stage(int16_t* dst, int k) const {
    uint2 o;
    if (bytes == 1) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(p + k);
      const uint32_t c0 = w & 0xffu, c1 = (w >> 8) & 0xffu, c2 = (w >> 16) & 0xffu, c3 = w >> 24;
      if (enc == WEKWS_HIP_WIRE_MULAW) o = pack(wire_mulaw(c0), wire_mulaw(c1), wire_mulaw(c2), wire_mulaw(c3));
      else if (enc == WEKWS_HIP_WIRE_ALAW) o = pack(wire_alaw(c0), wire_alaw(c1), wire_alaw(c2), wire_alaw(c3));
      else o = pack(wire_u8(c0), wire_u8(c1), wire_u8(c2), wire_u8(c3));
    } else if (bytes == 2) {
      o = *reinterpret_cast<const uint2*>(p + int64_t(k) * 2);
    } else {
      const uint4 a = *reinterpret_cast<const uint4*>(p + int64_t(k) * 4);
      o = pack(wire_f32(__uint_as_float(a.x)), wire_f32(__uint_as_float(a.y)), wire_f32(__uint_as_float(a.z)),
               wire_f32(__uint_as_float(a.w)));
    }
    *reinterpret_cast<uint2*>(dst) = o;
    return 0;
  }
};

// position rel of the row's virtual signal [history | chunk], zeros outside
template <typename Chunk>
__device__ __forceinline__ typename Chunk::Sample resample_fetch(const ResampleRow& R, const typename Chunk::Sample* hist,
                                                                 const Chunk& chunk, int rel) {
  typedef typename Chunk::Sample In;
  if (rel < 0 || rel >= R.hi_valid) return In(0);
  if constexpr (Chunk::kPlain) {             // one load through the chosen address, not a load under either branch
    const In* const q = rel < R.h ? hist + (R.hist_old + rel) : chunk.p + (rel - R.h);
    return *q;
  } else {
    return rel < R.h ? hist[R.hist_old + rel] : chunk.at(rel - R.h);
  }
}

template <typename Out>
__device__ __forceinline__ Out resample_out(float v) {
  if constexpr (std::is_same<Out, float>::value) {
    return v;
  } else {
    if (v != v) return Out(0);
    const float r = fminf(fmaxf(rintf(v), -32768.f), 32767.f);
    return Out(int(r));
  }
}

// The LDS of a workgroup under the plan P: the live table, the live ranges, the input tile.
template <typename In>
struct ResampleLds {
  float* taps;
  int* first;
  int* count;
  In* tile;
  __device__ __forceinline__ ResampleLds(unsigned char* lds, const ResampleParams& P)
      : taps(reinterpret_cast<float*>(lds)), first(reinterpret_cast<int*>(taps + P.n * P.stride)), count(first + P.n),
        tile(reinterpret_cast<In*>(lds + P.tile_off)) {}
};

// the live table and the live ranges of P into LDS (the caller's barrier follows)
template <typename In>
__device__ __forceinline__ void resample_load_table(const ResampleParams& P, const ResampleLds<In>& S) {
  const int tid = threadIdx.x;
  for (int e = tid; e < P.n * P.stride; e += kResampleTile) S.taps[e] = P.live[e];
  for (int e = tid; e < P.n; e += kResampleTile) { S.first[e] = P.first[e]; S.count[e] = P.count[e]; }
}

// Tile tl of row R, by the whole workgroup: the history write-back (tile 0), the staging, one output per lane.  src / yrow: the
// row's input (as Chunk reads it) and output.  Ends behind a barrier, so the next tile may overwrite the samples (and the table).
template <typename Chunk, typename Out>
__device__ __forceinline__ void resample_tile(const ResampleParams& P, const ResampleLds<typename Chunk::Sample>& S,
                                              const ResampleRow& R, const typename Chunk::Src* __restrict__ src,
                                              typename Chunk::Sample* hist, Out* __restrict__ yrow, int mcap, int tl) {
  typedef typename Chunk::Sample In;
  const Chunk chunk(src, R);
  constexpr int V = Chunk::kGroup;
  constexpr bool kFloatIn = std::is_same<In, float>::value;
  const float* const taps = S.taps;
  const int* const first = S.first;
  const int* const count = S.count;
  In* const tile = S.tile;
  const int tid = threadIdx.x;
  const int r0 = tl * kResampleTile, r = r0 + tid;
  if (tl == 0)
    for (int e = tid; e < R.keep_cnt; e += kResampleTile) hist[R.hist_new + e] = resample_fetch(R, hist, chunk, R.keep_from + e);
  if (r0 >= R.cnt) {                                           // (the whole workgroup: a tile past the row's count is zeros)
    if (r < mcap) yrow[r] = Out(0);
    return;
  }
  // ---- the samples under the full windows of the tile's outputs, from position tile_lo on
  const int jt0 = (R.i0 + r0) / P.n;
  int tile_lo = R.base_rel + jt0 * P.o;
  const int a = chunk.slack(tile_lo - R.h);                    // down to the alignment of the chunk's group loads
  tile_lo -= a;
  int bad = 0;
  for (int g = tid; g < P.tile_cap / V; g += kResampleTile) {
    const int rel = tile_lo + g * V;
    if (rel >= 0 && rel >= R.h && rel + V <= R.hi_valid) {
      bad |= chunk.stage(tile + g * V, rel - R.h);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const In s = resample_fetch(R, hist, chunk, rel + k);
        tile[g * V + k] = s;
        if constexpr (kFloatIn) bad |= resample_nonfinite(s);
      }
    }
  }
  if constexpr (kFloatIn) bad = __syncthreads_or(bad);
  else __syncthreads();
  // ---- one output per lane
  float acc = 0.f;
  const bool live = r < R.cnt;
  if (live) {
    const int qq = R.i0 + r, jj = qq / P.n, i = qq - jj * P.n;
    const In* const xs = tile + ((jj - jt0) * P.o + a);        // the sample under tap 0 of the output's block
    if (kFloatIn && bad) {
      const float* const k = P.full + int64_t(i) * P.K;
      for (int m = 0; m < P.K; ++m) acc = fmaf(k[m], float(xs[m]), acc);
    } else {
      acc = resample_sample(taps + i * P.stride, count[i], xs + first[i]);
    }
  }
  if (r < mcap) yrow[r] = live ? resample_out<Out>(acc) : Out(0);
  __syncthreads();                                             // the next tile overwrites the samples
}

template <typename In, typename Out>
__global__ __launch_bounds__(kResampleTile) void resample_kernel(const ResampleParams P, const ResampleRow* __restrict__ rows,
                                                                 const In* __restrict__ x, int64_t xstride, In* hist,
                                                                 Out* __restrict__ y, int mcap, int tiles_per_row,
                                                                 int64_t total_tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char resample_lds[];
  const ResampleLds<In> S(resample_lds, P);
  resample_load_table(P, S);
  __syncthreads();

  for (int64_t t = blockIdx.x; t < total_tiles; t += gridDim.x) {
    const int b = int(t / tiles_per_row), tl = int(t - int64_t(b) * tiles_per_row);
    const ResampleRow R = rows[b];
    resample_tile<ResampleChunk<In>, Out>(P, S, R, x + int64_t(b) * xstride, hist, y + int64_t(b) * mcap, mcap, tl);
  }
}

int launch_resample(const ResampleParams& P, size_t lds, int in_i16, int out_i16, const ResampleRow* rows, const void* x,
                    int64_t xstride, int16_t* hist, void* y, int B, int mcap, int max_grid, hipStream_t stream);

}  // namespace wekws

// (the handle of wekws_hip_resample_* is the rate bank's, with one member: resample_bank.hip.h)
