// The host plan of a RATE BANK: up to kResampleBankMax source rates resampled to one target rate by one launch
// (resample_bank.hip.h).  Pure host C++, no HIP, built on resample_plan.h: every member is the ResamplePlan of its pair with the
// bank's lowpass_filter_width and rolloff (a member equal to the target is the copy plan), and a row or a stream of member m is
// planned with exactly the functions a single-rate handle plans it with.
//
// Sizes of the bank are maxima over its members: the LDS of a launch, the history capacity of a stream (so a stream may change
// member without moving its buffers), max_out(nmax, flush).
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

namespace wekws {

constexpr int kResampleBankMax = 16;

struct ResampleBankPlan {
  int32_t neu = 0;
  std::vector<ResamplePlan> members;    // ranges only until resample_plan_taps is called on them
};

enum ResampleBankRefusal {
  kResampleBankOk = 0,
  kResampleBankCount,     // no member, or more than kResampleBankMax
  kResampleBankRate,      // a rate <= 0 (*bad: the member; -1: the target)
  kResampleBankRepeat,    // *bad repeats an earlier member
  kResampleBankParams,    // lowpass_filter_width / rolloff no resampler has
  kResampleBankLds,       // *bad's table does not fit the LDS budget
};

// The members' geometry and live ranges (no tap is computed), or the refusal and the member it is about.
inline ResampleBankRefusal resample_bank_plan(const int32_t* rates, int num, int neu, int lpw, double rolloff, ResampleBankPlan* bp,
                                              int* bad) {
  *bad = -1;
  if (!rates || num < 1 || num > kResampleBankMax) return kResampleBankCount;
  if (neu <= 0) return kResampleBankRate;
  for (int m = 0; m < num; ++m) {
    *bad = m;
    if (rates[m] <= 0) return kResampleBankRate;
    for (int k = 0; k < m; ++k)
      if (rates[k] == rates[m]) return kResampleBankRepeat;
  }
  bp->neu = neu;
  bp->members.assign(size_t(num), ResamplePlan());
  for (int m = 0; m < num; ++m) {
    *bad = m;
    ResamplePlan& p = bp->members[size_t(m)];
    if (resample_plan_ranges(rates[m], neu, lpw, rolloff, &p)) return kResampleBankParams;
    if (resample_lds_bytes(p) > kResampleLdsBudget || int64_t(p.n) * p.K > (int64_t(1) << 24)) return kResampleBankLds;
  }
  *bad = -1;
  return kResampleBankOk;
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
