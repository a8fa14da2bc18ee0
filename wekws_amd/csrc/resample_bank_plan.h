// The host plan of a RATE BANK: up to kResampleBankMax source rates resampled to one target rate by one launch
// (resample_bank.hip.h).  Pure host C++, no HIP, built on resample_plan.h: every member is the ResamplePlan of its pair with the
// bank's lowpass_filter_width and rolloff (a member equal to the target is the copy plan), and a row or a stream of member m is
// planned with exactly the functions a single-rate handle plans it with.
//
// Sizes of the bank are maxima over its members: the LDS of a launch, the history capacity of a stream (so a stream may change
// member without moving its buffers), max_out(nmax, flush).
//
// Wire encodings (wire.h).  A member is a (rate, encoding) pair: the bytes its rows arrive in, S16 unless the bank is created with
// encodings.  Two members may share a rate; a repeated PAIR is refused.  The encoding changes nothing above -- every encoding
// decodes to int16 in the kernel's fetch, the history stays int16 -- it decides how a row of a call is READ: a wire call
// (resample_bank_check_rows, wire_call = 1) takes rows of bytes, row b holding nsamp[b] samples of wire_bytes[member] bytes each,
// and a call in the kernel's own sample types (int16, float) may only name members that are S16.
//
// Tile order of a launch over B rows of tiles_per_row tiles each.  Rows keep their place in the input and in the output; what is
// ordered is the list of (row, tile) pairs the workgroups walk:
//   slots   order[s], s = 0..B-1: the rows sorted by member, rows of one member in their own order (a stable counting sort)
//   list    entry t = 0..B tiles_per_row - 1 is tile (t mod tiles_per_row) of row order[t div tiles_per_row]: all tiles of a member
//           are contiguous
//   spans   workgroup w of grid walks the entries [span_begin(w), span_begin(w + 1)): with total = q grid + r the first r spans hold
//           q + 1 entries and the others q -- contiguous, disjoint, covering the list.  A contiguous range of a list in which every
//           member is one run changes member at most members - 1 times; with many more tiles than members almost every span lies
//           inside one run and its workgroup loads one table.
#pragma once
#include <stdint.h>

#include <vector>

#include "resample_plan.h"
#include "wire.h"

namespace wekws {

constexpr int kResampleBankMax = 16;

struct ResampleBankPlan {
  int32_t neu = 0;
  std::vector<ResamplePlan> members;    // ranges only until resample_plan_taps is called on them
  std::vector<int32_t> wire, wire_bytes;  // of every member: enum wekws_hip_wire and the bytes of one sample
};

enum ResampleBankRefusal {
  kResampleBankOk = 0,
  kResampleBankCount,     // no member, or more than kResampleBankMax
  kResampleBankRate,      // a rate <= 0 (*bad: the member; -1: the target)
  kResampleBankRepeat,    // *bad repeats an earlier member
  kResampleBankParams,    // lowpass_filter_width / rolloff no resampler has
  kResampleBankLds,       // *bad's table does not fit the LDS budget
  kResampleBankWire,      // *bad's encoding is none of wire.h
};

// The members' geometry and live ranges (no tap is computed), or the refusal and the member it is about.
// encs: the members' encodings, or NULL: every member S16.
inline ResampleBankRefusal resample_bank_plan(const int32_t* rates, const int32_t* encs, int num, int neu, int lpw, double rolloff,
                                              ResampleBankPlan* bp, int* bad) {
  *bad = -1;
  if (!rates || num < 1 || num > kResampleBankMax) return kResampleBankCount;
  if (neu <= 0) return kResampleBankRate;
  for (int m = 0; m < num; ++m) {
    *bad = m;
    if (rates[m] <= 0) return kResampleBankRate;
    if (encs && !wire_sample_bytes(encs[m])) return kResampleBankWire;
    for (int k = 0; k < m; ++k)
      if (rates[k] == rates[m] && (!encs || encs[k] == encs[m])) return kResampleBankRepeat;
  }
  bp->neu = neu;
  bp->members.assign(size_t(num), ResamplePlan());
  bp->wire.assign(size_t(num), WEKWS_HIP_WIRE_S16);
  if (encs) bp->wire.assign(encs, encs + num);
  bp->wire_bytes.resize(size_t(num));
  for (int m = 0; m < num; ++m) bp->wire_bytes[size_t(m)] = wire_sample_bytes(bp->wire[size_t(m)]);
  for (int m = 0; m < num; ++m) {
    *bad = m;
    ResamplePlan& p = bp->members[size_t(m)];
    if (resample_plan_ranges(rates[m], neu, lpw, rolloff, &p)) return kResampleBankParams;
    if (resample_lds_bytes(p) > kResampleLdsBudget || int64_t(p.n) * p.K > (int64_t(1) << 24)) return kResampleBankLds;
  }
  *bad = -1;
  return kResampleBankOk;
}

inline ResampleBankRefusal resample_bank_plan(const int32_t* rates, int num, int neu, int lpw, double rolloff, ResampleBankPlan* bp,
                                              int* bad) {
  return resample_bank_plan(rates, nullptr, num, neu, lpw, rolloff, bp, bad);
}

// ---- the rows of a call, before anything else is planned.  members (B): the member of every row (a one-shot call's
// member_of_row; a push's, looked up per stream).  wire_call: pcm (B, width) bytes, row b nsamp[b] samples of its member's
// encoding (nsamp NULL: as many as width holds); otherwise pcm (B, width) samples of the kernel's own type, nsamp NULL = width.
// limit: the most samples a row may hold beside that (a push: max_chunk; none: 2^30 - 1).
constexpr int kResampleWireAlign = 4;     // of pcm and of row_bytes: every row starts on a dword
enum ResampleBankRowRefusal {
  kResampleRowsOk = 0,
  kResampleRowsAlign,      // wire call: pcm is not 4-byte aligned
  kResampleRowsWidth,      // wire call: row_bytes is no multiple of 4, negative or above 2^30 - 4
  kResampleRowsMember,     // *bad names a member outside the bank
  kResampleRowsLength,     // *bad: nsamp outside 0 .. limit, or more samples than the row holds
  kResampleRowsEncoding,   // *bad: a row of a member that is not S16 in a call that takes int16 / float samples
};
inline int64_t resample_bank_row_samples(const ResampleBankPlan& bp, int wire_call, int member, int64_t width) {
  return wire_call ? width / bp.wire_bytes[size_t(member)] : width;
}
inline ResampleBankRowRefusal resample_bank_check_rows(const ResampleBankPlan& bp, int wire_call, uint64_t pcm_addr, int64_t width,
                                                       const int32_t* nsamp, const int32_t* members, int B, int64_t limit, int* bad) {
  *bad = -1;
  if (wire_call) {
    if (width < 0 || width % kResampleWireAlign || width > 0x3ffffffcLL) return kResampleRowsWidth;
    if (pcm_addr % kResampleWireAlign) return kResampleRowsAlign;
  }
  const int M = int(bp.members.size());
  for (int b = 0; b < B; ++b) {
    *bad = b;
    const int m = members[b];
    if (m < 0 || m >= M) return kResampleRowsMember;
    if (!wire_call && bp.wire[size_t(m)] != WEKWS_HIP_WIRE_S16) return kResampleRowsEncoding;
    const int64_t holds = resample_bank_row_samples(bp, wire_call, m, width);
    const int64_t len = nsamp ? nsamp[b] : holds;
    if (len < 0 || len > limit || len > holds) return kResampleRowsLength;   // (len bytes <= width  <=>  len <= width div bytes)
  }
  *bad = -1;
  return kResampleRowsOk;
}

inline int64_t resample_bank_lds_bytes(const ResampleBankPlan& bp) {
  int64_t v = 0;
  for (const ResamplePlan& p : bp.members) { const int64_t b = resample_lds_bytes(p); v = b > v ? b : v; }
  return v;
}
// samples a stream may hold between two pushes, whatever its member (even, as a single-rate handle's)
inline int32_t resample_bank_hist_cap(const ResampleBankPlan& bp) {
  int32_t v = 0;
  for (const ResamplePlan& p : bp.members) { const int32_t c = (resample_hist_cap(p) + 1) & ~1; v = c > v ? c : v; }
  return v;
}
inline int64_t resample_bank_max_out(const ResampleBankPlan& bp, int64_t nmax, int flush) {
  int64_t v = 0;
  for (const ResamplePlan& p : bp.members) { const int64_t c = resample_max_out(p, nmax, flush); v = c > v ? c : v; }
  return v;
}

// ---- the tile order (constexpr: the kernel evaluates the same expressions)
// order (B): the rows sorted by member, stable.  Members outside 0..num-1 are the caller's to refuse first.
inline void resample_bank_order(const int32_t* member_of_row, int B, int num, int32_t* order) {
  int32_t at[kResampleBankMax + 1] = {};
  for (int b = 0; b < B; ++b) ++at[member_of_row[b] + 1];
  for (int m = 0; m < num; ++m) at[m + 1] += at[m];
  for (int b = 0; b < B; ++b) order[at[member_of_row[b]]++] = b;
}
constexpr int64_t resample_bank_total(int64_t B, int tiles_per_row) { return B * tiles_per_row; }
constexpr int resample_bank_slot(int64_t t, int tiles_per_row) { return int(t / tiles_per_row); }
constexpr int resample_bank_tile(int64_t t, int tiles_per_row) { return int(t % tiles_per_row); }
// the first list entry of workgroup w = 0..grid (w = grid: the end of the list)
constexpr int64_t resample_bank_span_begin(int64_t total, int64_t grid, int64_t w) {
  return (total / grid) * w + (w < total % grid ? w : total % grid);
}
// workgroups of a launch: no more than there are entries
constexpr int64_t resample_bank_grid(int64_t total, int64_t max_grid) { return total < max_grid ? total : (max_grid < 1 ? 1 : max_grid); }

}  // namespace wekws
