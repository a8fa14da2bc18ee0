// The per-stream host state of a resampler handle, and the plan of its calls.  Pure host C++, no HIP, built on resample_plan.h and
// resample_bank_plan.h.  Both handles (wekws_hip_resample_*, wekws_hip_resample_bank_*; resample_bank.hip) keep their streams here and
// nowhere else: a single-rate handle is a bank of one S16 member.
//
// A stream is four counts -- samples received, outputs emitted, the first sample it still keeps (origin), which of its two history
// buffers holds them (par) -- its member and whether it was flushed.  The counts ARE the state: a stream that has received nothing
// reads nothing of its device buffers, so a reset touches no device memory and no push reads the device.
//
// A push is planned whole (resample_streams_plan), then its rows are written (resample_streams_push_rows), then it is committed
// (resample_streams_commit).  A refused plan changes no stream.  Refusals are an enum and the row they are about, as the plan
// headers give them; the words are the caller's.
//
// Row: ResampleRow (resample.hip.h states its fields); a template parameter so that this header needs no device header.
#pragma once
#include <stdint.h>

#include <vector>

#include "resample_bank_plan.h"

namespace wekws {

enum ResampleStreamsRefusal {
  kResampleStreamsOk = 0,
  kResampleStreamsId,        // *bad names a stream outside 0..max_streams-1
  kResampleStreamsTwice,     // *bad names a stream an earlier row of the call named
  kResampleStreamsRows,      // resample_bank_check_rows refuses (ResampleStreams::rows says how; *bad is its row)
  kResampleStreamsFlushed,   // *bad's stream was flushed and not reset since
  kResampleStreamsInternal,  // *bad's plan lies outside the handle's buffers: a bug, never a caller's doing
  kResampleStreamsCap,       // some row yields need_cap > mcap samples (*bad: -1)
};

struct ResampleStreams {
  int32_t max_streams = 0, max_chunk = 0, hist_cap = 0;
  // which refusal a call with SEVERAL faults names.  false (the bank): ids of every row, then the rows, then the streams.  true (the
  // single-rate handle): all three row by row, so the fault of the earliest row.
  bool row_by_row = false;
  std::vector<int64_t> received, emitted, origin;
  std::vector<int32_t> par, flushed, member;
  // ---- scratch of the call being planned; carries nothing from one call to the next (a refused call may leave it advanced)
  std::vector<int32_t> seen;             // == epoch: the call has named this stream
  int32_t epoch = 0;
  std::vector<ResampleStep> steps;       // of every row
  std::vector<int32_t> members_of, pos;  // of every row: its member, its slot in the uploaded table
  int64_t need_cap = 0;                  // most outputs of a row (of a call planned to its end)
  ResampleBankRowRefusal rows = kResampleRowsOk;
};

inline void resample_streams_init(ResampleStreams* s, int max_streams, int max_chunk, int hist_cap, bool row_by_row) {
  const size_t ns = size_t(max_streams);
  s->max_streams = max_streams; s->max_chunk = max_chunk; s->hist_cap = hist_cap; s->row_by_row = row_by_row;
  s->received.assign(ns, 0); s->emitted.assign(ns, 0); s->origin.assign(ns, 0);
  s->par.assign(ns, 0); s->flushed.assign(ns, 0); s->member.assign(ns, 0); s->seen.assign(ns, 0);
  s->steps.reserve(ns);
}

// The slot of every row in the uploaded table: the rows sorted by member, stable -- the inverse of resample_bank_order.  A bank of
// one member keeps row order; NULL is then returned and a row's slot is its index.
inline const int32_t* resample_slot_positions(ResampleStreams* s, const int32_t* member_of_row, int B, int num) {
  if (num < 2) return nullptr;
  int32_t at[kResampleBankMax + 1] = {};
  for (int b = 0; b < B; ++b) ++at[member_of_row[b] + 1];
  for (int m = 0; m < num; ++m) at[m + 1] += at[m];
  s->pos.resize(size_t(B));
  for (int b = 0; b < B; ++b) s->pos[size_t(b)] = at[member_of_row[b]]++;
  return s->pos.data();
}

// A push of B rows, row b nsamp[b] samples for stream ids[b] (flush: and every one of them ends), into mcap outputs per row.
// wire_call, pcm_addr, width: as resample_bank_check_rows takes them; the rows' limit is max_chunk.
inline ResampleStreamsRefusal resample_streams_plan(ResampleStreams* s, const ResampleBankPlan& bp, int wire_call, uint64_t pcm_addr,
                                                    int64_t width, const int32_t* ids, const int32_t* nsamp, int B, int flush,
                                                    int64_t mcap, int* bad) {
  if (++s->epoch == 0x7fffffff) { s->epoch = 1; s->seen.assign(s->seen.size(), 0); }
  s->steps.resize(size_t(B));
  s->members_of.resize(size_t(B));
  s->need_cap = 0;
  s->rows = kResampleRowsOk;
  // (locals: what the loops read of *s must not look as if the loops' own stores could change it)
  const int32_t epoch = s->epoch, max_streams = s->max_streams, hist_cap = s->hist_cap;
  const int64_t* const received = s->received.data();
  const int64_t* const emitted = s->emitted.data();
  const int64_t* const origin = s->origin.data();
  const int32_t* const member = s->member.data();
  const int32_t* const flushed = s->flushed.data();
  int32_t* const seen = s->seen.data();
  int32_t* const members_of = s->members_of.data();
  ResampleStep* const steps = s->steps.data();
  const ResamplePlan* const plans = bp.members.data();
  const int64_t limit = s->max_chunk;
  int64_t need_cap = 0;
  // ---- the three looks at row b (inlined where they are used: as calls they would take every local above through a pointer)
  auto name_stream = [&](int b) __attribute__((always_inline)) {
    const int id = ids[b];
    if (id < 0 || id >= max_streams) return kResampleStreamsId;
    if (seen[id] == epoch) return kResampleStreamsTwice;
    seen[id] = epoch;
    members_of[b] = member[id];
    return kResampleStreamsOk;
  };
  // (the rows as their streams' members read them: lengths in samples against max_chunk and against what the row holds)
  auto check_rows = [&](int b0, int rows) __attribute__((always_inline)) {
    int at = -1;
    const ResampleBankRowRefusal rr = resample_bank_check_rows(bp, wire_call, pcm_addr, width, nsamp + b0, members_of + b0, rows, limit, &at);
    if (rr == kResampleRowsOk) return kResampleStreamsOk;
    s->rows = rr;
    *bad = at < 0 ? at : at + b0;
    return kResampleStreamsRows;
  };
  auto step_stream = [&](int b) __attribute__((always_inline)) {
    const int id = ids[b];
    if (flushed[id]) return kResampleStreamsFlushed;
    const ResampleStep st = resample_step(plans[members_of[b]], received[id], nsamp[b], flush);
    const int64_t N2 = received[id] + nsamp[b];
    if (N2 - st.keep_from > hist_cap || st.keep_from < origin[id] || st.total < emitted[id]) return kResampleStreamsInternal;
    if (st.total - emitted[id] > need_cap) need_cap = st.total - emitted[id];
    steps[b] = st;
    return kResampleStreamsOk;
  };
  // ---- in the handle's order
  ResampleStreamsRefusal r = kResampleStreamsOk;
  if (s->row_by_row) {
    for (int b = 0; b < B; ++b) {
      if ((r = name_stream(b)) != kResampleStreamsOk) { *bad = b; return r; }
      if ((r = check_rows(b, 1)) != kResampleStreamsOk) return r;
      if ((r = step_stream(b)) != kResampleStreamsOk) { *bad = b; return r; }
    }
  } else {
    for (int b = 0; b < B; ++b)
      if ((r = name_stream(b)) != kResampleStreamsOk) { *bad = b; return r; }
    if ((r = check_rows(0, B)) != kResampleStreamsOk) return r;
    for (int b = 0; b < B; ++b)
      if ((r = step_stream(b)) != kResampleStreamsOk) { *bad = b; return r; }
  }
  *bad = -1;
  s->need_cap = need_cap;
  return need_cap > mcap ? kResampleStreamsCap : kResampleStreamsOk;
}

// The rows of the planned push, row b to table[pos[b]] (pos NULL: table[b]): the stream's [history | chunk] continued at its next
// output.
template <typename Row>
inline void resample_streams_push_rows(const ResampleStreams& s, const ResampleBankPlan& bp, int wire_call, const int32_t* ids,
                                       const int32_t* nsamp, int B, const int32_t* pos, Row* table) {
  // (locals: a row's stores must not look as if they could move the arrays)
  const int64_t* const received = s.received.data();
  const int64_t* const emitted = s.emitted.data();
  const int64_t* const origin = s.origin.data();
  const int32_t* const par = s.par.data();
  const int32_t* const members_of = s.members_of.data();
  const ResampleStep* const steps = s.steps.data();
  const ResamplePlan* const plans = bp.members.data();
  const int32_t* const wire = bp.wire.data();
  const int32_t hist_cap = s.hist_cap;
  for (int b = 0; b < B; ++b) {
    const int id = ids[b], m = members_of[b];
    const ResamplePlan& p = plans[m];
    const ResampleStep st = steps[b];
    const int64_t q0 = emitted[id], j0 = q0 / p.n, s0 = origin[id], N = received[id];
    Row R{};
    R.i0 = int32_t(q0 - j0 * p.n);
    R.base_rel = int32_t(j0 * p.o - p.width - s0);
    R.cnt = int32_t(st.total - q0);
    R.h = int32_t(N - s0);
    R.hi_valid = R.h + nsamp[b];
    R.hist_old = (id * 2 + par[id]) * hist_cap;
    R.hist_new = (id * 2 + (par[id] ^ 1)) * hist_cap;
    R.keep_from = int32_t(st.keep_from - s0);
    R.keep_cnt = int32_t(N + nsamp[b] - st.keep_from);
    R.member = m; R.row = b;
    R.wire = wire_call ? wire[m] : 0;
    table[pos ? pos[b] : b] = R;
  }
}

// Row b of a one-shot call: an utterance of len samples at member m's rate, from its first sample.  Returns its outputs.
inline int64_t resample_once_count(const ResampleBankPlan& bp, int m, int64_t len) { return resample_num_samples(bp.members[size_t(m)], len); }
template <typename Row>
inline void resample_once_row(const ResampleBankPlan& bp, int wire_call, int m, int b, int32_t len, Row* out) {
  Row& R = *out;
  R = Row{};
  R.base_rel = -bp.members[size_t(m)].width;
  R.cnt = int32_t(resample_once_count(bp, m, len));
  R.hi_valid = len;
  R.member = m; R.row = b;
  R.wire = wire_call ? bp.wire[size_t(m)] : 0;
}

// The planned push is done (launched): what every row yielded, and the streams move.
inline void resample_streams_commit(ResampleStreams* s, const int32_t* ids, const int32_t* nsamp, int B, int flush, int32_t* counts) {
  for (int b = 0; b < B; ++b) {
    const size_t id = size_t(ids[b]);
    const ResampleStep& st = s->steps[size_t(b)];
    counts[b] = int32_t(st.total - s->emitted[id]);
    s->received[id] += nsamp[b];
    s->emitted[id] = st.total;
    s->origin[id] = st.keep_from;
    s->par[id] ^= 1;
    if (flush) s->flushed[id] = 1;
  }
}

// The streams ids (n) start over, as member `member` (-1: as the member each one is).  -1, or the index of the first id outside
// 0..max_streams-1: then no stream has changed.
inline int resample_streams_reset(ResampleStreams* s, const int32_t* ids, int n, int member) {
  for (int i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= s->max_streams) return i;
  for (int i = 0; i < n; ++i) {
    const size_t id = size_t(ids[i]);
    if (member >= 0) s->member[id] = member;
    s->received[id] = 0; s->emitted[id] = 0; s->origin[id] = 0; s->flushed[id] = 0;
  }
  return -1;
}

// received, emitted, kept, flushed
inline void resample_streams_counts(const ResampleStreams& s, int id, int64_t out[4]) {
  const size_t k = size_t(id);
  out[0] = s.received[k]; out[1] = s.emitted[k]; out[2] = s.received[k] - s.origin[k]; out[3] = s.flushed[k];
}

}  // namespace wekws
