// The resampler for rows of DIFFERENT source rates in one launch: a rate bank (resample_bank_plan.h) of up to 16 members, each the
// plan of one (orig, new) pair.  The arithmetic, the staging, the non-finite path and the history write-back are the single-rate
// kernel's own device functions (resample.hip.h: resample_tile and what it calls), given the parameters of the row's member: a
// row's output equals the single-rate kernel's for that rate bit for bit.
//
//   workgroup   256 lanes, one output per lane; persistent over ONE CONTIGUOUS SPAN of the (row, tile) list, which is ordered by
//               member (resample_bank_plan.h states the order and the spans).
//   table       the parameters of every member (ResampleParams: sizes, LDS offsets, table pointers) are a small device table.  The
//               workgroup remembers which member's live table and live ranges its LDS holds; when its next tile is of another
//               member it passes a barrier (other waves may still read the old table), reloads, and passes a second one.  A span
//               changes member at most members - 1 times, and usually never.
//   LDS         the layout of the loaded member, exactly as the single-rate kernel lays it out; the launch asks for the largest
//               member's bytes.
//   rows        the row table is uploaded in slot order (sorted by member); a row carries its member and its place in x and y.
//   wire        a third source beside int16 and float rows: rows of BYTES in their member's wire encoding (wire.h), decoded to int16
//               in the fetch (resample.hip.h: ResampleWireChunk).  x is then (B, xstride) bytes and the row carries its encoding; the
//               history, the LDS tile and the arithmetic are the int16 rows'.  The list is ordered by member, so the encoding is
//               uniform over a workgroup's current row.
#pragma once
#include "resample.hip.h"
#include "resample_bank_plan.h"
#include "resample_streams.h"

namespace wekws {

template <typename Chunk, typename Out>
__global__ __launch_bounds__(kResampleTile) void resample_bank_kernel(const ResampleParams* __restrict__ members,
                                                                      const ResampleRow* __restrict__ rows,
                                                                      const typename Chunk::Src* __restrict__ x, int64_t xstride,
                                                                      typename Chunk::Sample* hist, Out* __restrict__ y, int mcap,
                                                                      int tiles_per_row, int64_t total_tiles) {
  typedef typename Chunk::Sample In;
  extern __shared__ __attribute__((aligned(16))) unsigned char resample_bank_lds[];
  const int64_t t0 = resample_bank_span_begin(total_tiles, gridDim.x, blockIdx.x);
  const int64_t t1 = resample_bank_span_begin(total_tiles, gridDim.x, int64_t(blockIdx.x) + 1);
  int loaded = -1;
  ResampleParams P{};
  for (int64_t t = t0; t < t1; ++t) {
    const ResampleRow R = rows[resample_bank_slot(t, tiles_per_row)];
    if (R.member != loaded) {
      __syncthreads();                                           // other waves may still read the old table
      P = members[R.member];
      resample_load_table(P, ResampleLds<In>(resample_bank_lds, P));
      loaded = R.member;
      __syncthreads();
    }
    resample_tile<Chunk, Out>(P, ResampleLds<In>(resample_bank_lds, P), R, x + int64_t(R.row) * xstride, hist,
                              y + int64_t(R.row) * mcap, mcap, resample_bank_tile(t, tiles_per_row));
  }
}

enum ResampleBankSource { kResampleBankF32 = 0, kResampleBankI16 = 1, kResampleBankWireBytes = 2 };   // what x holds; xstride in its units
int launch_resample_bank(const ResampleParams* members, size_t lds, int source, int out_i16, const ResampleRow* rows, const void* x,
                         int64_t xstride, int16_t* hist, void* y, int B, int mcap, int max_grid, hipStream_t stream);

}  // namespace wekws

// The host handle of wekws_hip_resample_* AND of wekws_hip_resample_bank_* (resample_bank.hip holds everything that works on it; the
// hooks unit caps its grid and rounds a member's tables).  A single-rate handle is this struct with one S16 member: the bank's sizes are
// maxima over one plan.  It differs in `kind` alone -- which kernel a call launches and which name its messages carry.
struct wekws_hip_resample {
  enum Kind { kSingle = 0, kBank = 1 };
  int kind = kBank;
  int device = 0;
  wekws::ResampleBankPlan bank;                    // (a member's rate: bank.members[m].orig; its encoding: bank.wire[m])
  std::vector<wekws::ResampleParams> P;            // of every member, as the device table holds them
  wekws::ResampleParams* d_params = nullptr;
  size_t lds = 0;
  int out_i16 = 0, max_grid = 1, default_grid = 1;
  std::vector<float*> d_live, d_full;              // per member
  std::vector<int32_t*> d_meta;                    // per member: first (n) | count (n)
  int16_t* hist = nullptr;                         // (max_streams, 2, hist_cap) kept samples, ping-ponged per stream
  // The row table of EVERY call, one-shot or push, travels through one ring of pinned host tables, each with its device twin and an
  // event recorded behind the call that used it: calls queue back to back without a synchronise.  Slots are allocated for max_streams
  // rows at create (a push never has more); a one-shot call with more rows replaces its slot.
  struct Slot {
    wekws::ResampleRow* h = nullptr;
    wekws::ResampleRow* d = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool used = false;
  };
  Slot ring[wekws::kResampleRing];
  int next = 0;
  std::mutex mu;
  wekws::ResampleStreams streams;                  // per-stream state lives on the host: no call reads the device back
  const char* name() const { return kind == kSingle ? "resample" : "resample_bank"; }
};

namespace wekws {

// what the C entry points of both families are (resample.hip, resample_bank.hip); h: a wekws_hip_resample
int resample_create(int kind, const wekws_hip_resample_cfg* cfg, const int32_t* rates, const int32_t* encs, int num, void** out);
void resample_destroy(void* h);
int resample_max_out(void* h, int nmax, int flush);
// member_of_row: NULL on a single-rate handle (every row member 0)
int resample_compute(void* h, int source, const void* pcm, int B, int width, const int32_t* nsamp, const int32_t* member_of_row, void* out,
                     int mcap, void* stream);
int resample_push(void* h, int wire_call, const void* pcm, int B, int width, const int32_t* stream_ids, const int32_t* nsamp, int flush,
                  void* out, int mcap, int32_t* counts, void* stream);
// member: NULL for reset (every stream stays the member it is), or set_rate's
int resample_reset(void* h, const int32_t* ids, int n, const int* member);
int resample_counts(void* h, int id, int64_t counts_out[4]);

}  // namespace wekws

