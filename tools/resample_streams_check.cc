// The stream planner of the resampler handles (wekws_amd/csrc/resample_streams.h) under the host sanitizers: a stand-alone program,
// no device, no Python.  It drives a seeded schedule of pushes -- shuffled rows of 0..max_chunk samples, a reset and a set_rate
// mid-way, refused calls in between, a flush at the end -- over a three-member bank and over a one-member bank planned as the
// single-rate handle plans, and holds what needs no reference: a refused call changes no stream, the uploaded table is a permutation
// of the rows sorted by member, every row lies inside the handle's buffers, and the counts add up.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I wekws_amd/csrc tools/resample_streams_check.cc -o rsc && ./rsc
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "resample_streams.h"

namespace {

struct Row { int32_t i0, base_rel, cnt, h, hi_valid, hist_old, hist_new, keep_from, keep_cnt, member, row, wire; };

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {                                   // 0..n-1 (xorshift64*)
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return uint32_t((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

std::vector<int64_t> all_counts(const wekws::ResampleStreams& S) {
  std::vector<int64_t> v(size_t(S.max_streams) * 4);
  for (int id = 0; id < S.max_streams; ++id) wekws::resample_streams_counts(S, id, &v[size_t(id) * 4]);
  return v;
}

int run(const std::vector<int32_t>& rates, bool single) {
  const int ns = 5, max_chunk = 700, num = int(rates.size());
  wekws::ResampleBankPlan bp;
  int bad = -1;
  CHECK(wekws::resample_bank_plan(rates.data(), num, 16000, 6, 0.99, &bp, &bad) == wekws::kResampleBankOk);
  wekws::ResampleStreams S;
  wekws::resample_streams_init(&S, ns, max_chunk, wekws::resample_bank_hist_cap(bp), single);
  for (int id = 0; id < ns; ++id) CHECK(wekws::resample_streams_reset(&S, &id, 1, id % num) == -1);
  int accepted = 0, refused = 0;
  auto refuse = [&](std::vector<int32_t> ids, std::vector<int32_t> nsamp, int width, int flush, int64_t mcap, int want, int want_row) {
    const std::vector<int64_t> before = all_counts(S);
    const int r = wekws::resample_streams_plan(&S, bp, 0, 0, width, ids.data(), nsamp.data(), int(ids.size()), flush, mcap, &bad);
    CHECK(r == want && bad == want_row && all_counts(S) == before);
    ++refused;
  };
  for (int k = 0; k < 12; ++k) {
    const bool last = k == 11;
    std::vector<int32_t> ids, nsamp;
    for (int id = 0; id < ns; ++id)
      if (!S.flushed[size_t(id)] && (last || rnd(3))) ids.insert(ids.begin() + rnd(uint32_t(ids.size()) + 1), id);
    for (size_t b = 0; b < ids.size(); ++b) nsamp.push_back(int32_t(rnd(max_chunk + 1)));
    const int B = int(ids.size());
    const std::vector<int64_t> before = all_counts(S);
    CHECK(wekws::resample_streams_plan(&S, bp, 0, 0, max_chunk, ids.data(), nsamp.data(), B, last, 4000, &bad) == wekws::kResampleStreamsOk);
    std::vector<Row> table(size_t(B), Row{-1, 0, 0, 0, 0, 0, 0, 0, 0, -1, -1, -1});
    std::vector<int32_t> yields(size_t(B), -1);
    const int32_t* pos = wekws::resample_slot_positions(&S, S.members_of.data(), B, num);
    CHECK((pos == nullptr) == (num == 1));
    std::vector<char> taken(size_t(B), 0);
    for (int b = 0; b < B; ++b) {
      const int at = pos ? pos[b] : b;
      CHECK(at >= 0 && at < B && !taken[size_t(at)]);
      taken[size_t(at)] = 1;
    }
    wekws::resample_streams_push_rows(S, bp, 0, ids.data(), nsamp.data(), B, pos, table.data());
    wekws::resample_streams_commit(&S, ids.data(), nsamp.data(), B, last, yields.data());
    const std::vector<int64_t> after = all_counts(S);
    for (int k2 = 0; k2 < B; ++k2) {
      const Row& R = table[size_t(k2)];
      const int b = R.row, id = ids[size_t(b)];
      CHECK(k2 == 0 || table[size_t(k2 - 1)].member < R.member || (table[size_t(k2 - 1)].member == R.member && table[size_t(k2 - 1)].row < b));
      CHECK(R.member == S.member[size_t(id)] && R.wire == 0 && R.cnt == yields[size_t(b)] && R.cnt <= S.need_cap);
      CHECK(R.i0 >= 0 && R.i0 < bp.members[size_t(R.member)].n && R.h >= 0 && R.h <= S.hist_cap && R.hi_valid == R.h + nsamp[size_t(b)]);
      CHECK(R.keep_from >= 0 && R.keep_cnt >= 0 && R.keep_cnt <= S.hist_cap && R.keep_from + R.keep_cnt == R.hi_valid);
      CHECK(R.hist_old / S.hist_cap / 2 == id && R.hist_new / S.hist_cap / 2 == id && R.hist_old != R.hist_new);
      CHECK(after[size_t(id) * 4] == before[size_t(id) * 4] + nsamp[size_t(b)] && after[size_t(id) * 4 + 1] == before[size_t(id) * 4 + 1] + R.cnt);
      CHECK(after[size_t(id) * 4 + 2] == R.keep_cnt && after[size_t(id) * 4 + 3] == last);
    }
    ++accepted;
    // ---- refused calls in between
    if (k == 0) refuse({1, ns, 0}, {5, 5, 5}, max_chunk, 0, 4000, wekws::kResampleStreamsId, 1);
    if (k == 1) refuse({2, 0, 3, 0}, {5, 5, 5, 5}, max_chunk, 0, 4000, wekws::kResampleStreamsTwice, 3);
    if (k == 2) refuse({4, 2}, {10, 601}, 600, 0, 4000, wekws::kResampleStreamsRows, 1);
    if (k == 3) refuse({0, 1, 3}, {700, 700, 701}, 800, 0, 4000, wekws::kResampleStreamsRows, 2);
    if (k == 4) {
      const std::vector<int32_t> four = {3, 1, 4, 0}, len = {700, 300, 0, 650};
      CHECK(wekws::resample_streams_plan(&S, bp, 0, 0, max_chunk, four.data(), len.data(), 4, 0, 4000, &bad) == wekws::kResampleStreamsOk);
      const int64_t need = S.need_cap;                                                      // (a plan that is not committed changes nothing)
      CHECK(need > 1);
      refuse(four, len, max_chunk, 0, need - 1, wekws::kResampleStreamsCap, -1);
    }
    if (k == 5) {
      const int32_t two = 2, three = 3;
      CHECK(wekws::resample_streams_reset(&S, &two, 1, -1) == -1 && wekws::resample_streams_reset(&S, &three, 1, num - 1) == -1);
      const int32_t outside[2] = {1, ns};
      const std::vector<int64_t> was = all_counts(S);
      CHECK(wekws::resample_streams_reset(&S, outside, 2, -1) == 1 && all_counts(S) == was);
    }
    if (k == 6) {
      const int32_t four = 4, len = 123;
      int32_t y = 0;
      CHECK(wekws::resample_streams_plan(&S, bp, 0, 0, max_chunk, &four, &len, 1, 1, 4000, &bad) == wekws::kResampleStreamsOk);
      wekws::resample_streams_commit(&S, &four, &len, 1, 1, &y);
      refuse({0, 4}, {5, 5}, max_chunk, 0, 4000, wekws::kResampleStreamsFlushed, 1);
    }
    if (k == 7) {
      const int32_t four = 4;
      CHECK(wekws::resample_streams_reset(&S, &four, 1, -1) == -1);
    }
  }
  CHECK(accepted == 12 && refused == 6);
  for (int id = 0; id < ns; ++id) CHECK(S.flushed[size_t(id)]);
  return 0;
}

}  // namespace

int main() {
  run({8000, 44100, 48000}, false);
  run({44100}, true);
  std::puts("resample_streams_check: ok");
  return 0;
}
