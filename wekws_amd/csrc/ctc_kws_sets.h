// The keyword sets of a CTC decoder handle: what `KeyWordSpotter.set_keywords` (wekws/bin/stream_kws_ctc.py:304-333) gives ONE
// spotter object, kept as a registry so that every stream of a batched handle can have its own.  Pure host C++, no HIP: this
// table decides every refusal, hands out the ids, lays out the device tables and mirrors the streams' assignments; the
// launchers (ctc_kws.hip) upload what it wrote, the kernels (ctc_kws.hip.h) read one record per wave.
//
// A set is a list of keywords (token-id sequences, insertion order, each non-empty; none at all is allowed), a first-beam
// token set or none, and a threshold.  Set 0 is the first one added (the handle's descriptor) and is never dropped; every
// stream starts in it.
//
// Device tables, and their images here:
//   recs   one CtcSetRec per set id
//   kw     int32 arena.  A set's block: n_kw + 1 offsets, relative to the block's first token, then the tokens -- the layout
//          the descriptor's own keywords always had, so the detection loop indexes it unchanged
//   mask   uint32 arena of blocks of W = ceil(V / 32) words: bit s of a block = token s is in the set
//   stream_set   the set id of every stream
// A dropped set gives its id, its block and its mask back: the lowest free id is handed out first, blocks first-fit from the
// lowest address (neighbouring free blocks merge), masks lowest first.  The arenas never shrink, so a record of a dropped id
// still points inside them; no stream can be assigned to it.
#pragma once
#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

namespace wekws {

struct CtcSetRec {     // 24 bytes; the device reads it as it is
  int32_t kw_base;     // the set's block in the keyword arena
  int32_t n_kw;
  int32_t mask_word;   // word offset of its mask in the mask arena, -1 = no token set
  int32_t reserved;
  double threshold;
};

struct CtcSetSpec {    // as wekws_hip_ctc_kws_desc gives them; token_set NULL = no first-beam set, whatever token_set_len says
  const int32_t* tokens;
  const int32_t* offsets;
  int num_keywords;
  const int32_t* token_set;
  int token_set_len;
  double threshold;
};

class CtcSetTable {
 public:
  int V = 0, W = 0, n_streams = 0;
  std::vector<CtcSetRec> recs;       // index: set id, up to the highest id ever handed out
  std::vector<uint8_t> live;
  std::vector<int32_t> users;        // streams assigned to the set
  std::vector<int32_t> kw;
  std::vector<uint32_t> mask;
  std::vector<int32_t> stream_set;

  void init(int vocab, int streams) {
    V = vocab; W = (vocab + 31) / 32; n_streams = streams;
    recs.clear(); live.clear(); users.clear(); kw.clear(); mask.clear(); kw_free_.clear(); mask_free_.clear();
    stream_set.assign(size_t(streams), 0);
    seen_.assign(size_t(streams), 0);
    epoch_ = 0;
  }

  bool known(int set) const { return set >= 0 && size_t(set) < recs.size() && live[size_t(set)]; }
  int set_of(int id) const { return id >= 0 && id < n_streams ? stream_set[size_t(id)] : -1; }
  // ints of the set's block in the keyword arena
  int32_t kw_len(int set) const {
    const CtcSetRec& r = recs[size_t(set)];
    return r.n_kw + 1 + kw[size_t(r.kw_base) + size_t(r.n_kw)];
  }

  // 0, or -1 with the reason in `why`: what no set may look like
  int check(const CtcSetSpec& s, char* why, size_t n) const {
    if (s.num_keywords < 0 || s.token_set_len < 0) return say(why, n, "num_keywords=%d token_set_len=%d", s.num_keywords, s.token_set_len);
    if (s.num_keywords > 0 && (!s.tokens || !s.offsets)) return say(why, n, "keywords given without tokens / offsets");
    if (s.num_keywords > 0 && s.offsets[0] != 0) return say(why, n, "keyword_offsets[0] must be 0");
    for (int k = 0; k < s.num_keywords; ++k)
      if (s.offsets[k + 1] <= s.offsets[k]) return say(why, n, "keyword %d is empty (offsets must increase)", k);
    const int total = s.num_keywords > 0 ? s.offsets[s.num_keywords] : 0;
    for (int i = 0; i < total; ++i)
      if (s.tokens[i] < 0 || s.tokens[i] >= V) return say(why, n, "keyword token %d outside the vocabulary (%d)", s.tokens[i], V);
    for (int i = 0; s.token_set && i < s.token_set_len; ++i)
      if (s.token_set[i] < 0 || s.token_set[i] >= V) return say(why, n, "token set entry %d outside the vocabulary", s.token_set[i]);
    return 0;
  }

  // the new set's id (the lowest free one), or -1: nothing changed
  int add(const CtcSetSpec& s, char* why, size_t n) {
    if (check(s, why, n)) return -1;
    const int total = s.num_keywords > 0 ? s.offsets[s.num_keywords] : 0;
    const int64_t len = int64_t(s.num_keywords) + 1 + total;
    size_t id = 0;
    while (id < recs.size() && live[id]) ++id;
    if (len > 0x3fffffff || id >= 0x3fffffff) { say(why, n, "the set is too large"); return -1; }
    const int64_t at = take_kw(int32_t(len));
    if (at < 0) { say(why, n, "the keyword arena is full"); return -1; }
    int32_t mw = -1;
    if (s.token_set) {
      mw = take_mask();
      if (mw < 0) { give_kw(int32_t(at), int32_t(len)); say(why, n, "the mask arena is full"); return -1; }
      uint32_t* m = mask.data() + mw;
      std::memset(m, 0, size_t(W) * 4);
      for (int i = 0; i < s.token_set_len; ++i) m[s.token_set[i] >> 5] |= 1u << (s.token_set[i] & 31);
    }
    int32_t* b = kw.data() + at;
    b[0] = 0;
    for (int k = 0; k < s.num_keywords; ++k) b[k + 1] = s.offsets[k + 1];
    for (int i = 0; i < total; ++i) b[s.num_keywords + 1 + i] = s.tokens[i];
    if (id == recs.size()) { recs.push_back(CtcSetRec{}); live.push_back(0); users.push_back(0); }
    recs[id] = CtcSetRec{int32_t(at), s.num_keywords, mw, 0, s.threshold};
    live[id] = 1;
    users[id] = id == 0 ? n_streams : 0;
    return int(id);
  }

  // 0, or -1: nothing changed
  int drop(int set, char* why, size_t n) {
    if (set == 0) return say(why, n, "set 0 is the handle's own and cannot be dropped");
    if (!known(set)) return say(why, n, "set %d is not registered", set);
    if (users[size_t(set)] > 0) return say(why, n, "set %d is in use by %d streams", set, users[size_t(set)]);
    const CtcSetRec r = recs[size_t(set)];
    give_kw(r.kw_base, kw_len(set));
    if (r.mask_word >= 0) mask_free_.push_back(r.mask_word);
    recs[size_t(set)] = CtcSetRec{0, 0, -1, 0, 0.0};
    live[size_t(set)] = 0;
    return 0;
  }

  // may streams ids[i] (distinct) take sets[i]?  0, or -1
  int assign_check(const int32_t* ids, const int32_t* sets, int count, char* why, size_t n) {
    if (count < 0 || (count > 0 && (!ids || !sets))) return say(why, n, "n=%d", count);
    if (++epoch_ == 0x7fffffff) { epoch_ = 1; seen_.assign(seen_.size(), 0); }
    for (int i = 0; i < count; ++i) {
      if (ids[i] < 0 || ids[i] >= n_streams) return say(why, n, "entry %d: stream %d outside 0..%d", i, ids[i], n_streams - 1);
      if (seen_[size_t(ids[i])] == epoch_) return say(why, n, "entry %d: stream %d is given twice", i, ids[i]);
      seen_[size_t(ids[i])] = epoch_;
      if (!known(sets[i])) return say(why, n, "entry %d: set %d is not registered", i, sets[i]);
    }
    return 0;
  }
  void assign_commit(const int32_t* ids, const int32_t* sets, int count) {
    for (int i = 0; i < count; ++i) {
      int32_t& cur = stream_set[size_t(ids[i])];
      --users[size_t(cur)];
      cur = sets[i];
      ++users[size_t(cur)];
    }
  }
  int assign(const int32_t* ids, const int32_t* sets, int count, char* why, size_t n) {
    if (assign_check(ids, sets, count, why, n)) return -1;
    assign_commit(ids, sets, count);
    return 0;
  }

  // The whole table as int32 (the hooks library's debug entry point returns it): ids, kw ints, mask words, streams; per id
  // live, users, kw_base, n_kw, mask_word and the threshold's two halves (low first); the kw arena; the mask arena; stream_set.
  std::vector<int32_t> image() const {
    std::vector<int32_t> o{int32_t(recs.size()), int32_t(kw.size()), int32_t(mask.size()), n_streams};
    for (size_t i = 0; i < recs.size(); ++i) {
      int32_t t[2];
      std::memcpy(t, &recs[i].threshold, 8);
      const int32_t v[7] = {live[i], users[i], recs[i].kw_base, recs[i].n_kw, recs[i].mask_word, t[0], t[1]};
      o.insert(o.end(), v, v + 7);
    }
    o.insert(o.end(), kw.begin(), kw.end());
    for (uint32_t m : mask) o.push_back(int32_t(m));
    o.insert(o.end(), stream_set.begin(), stream_set.end());
    return o;
  }

 private:
  struct Range { int32_t at, len; };
  std::vector<Range> kw_free_;        // ascending, no two adjacent
  std::vector<int32_t> mask_free_;
  std::vector<int32_t> seen_;
  int32_t epoch_ = 0;

  __attribute__((format(printf, 3, 4))) static int say(char* why, size_t n, const char* fmt, ...) {
    if (why && n > 0) {
      va_list ap;
      va_start(ap, fmt);
      vsnprintf(why, n, fmt, ap);
      va_end(ap);
    }
    return -1;
  }
  int64_t take_kw(int32_t len) {
    for (size_t i = 0; i < kw_free_.size(); ++i)
      if (kw_free_[i].len >= len) {
        const int32_t at = kw_free_[i].at;
        kw_free_[i].at += len; kw_free_[i].len -= len;
        if (!kw_free_[i].len) kw_free_.erase(kw_free_.begin() + long(i));
        return at;
      }
    if (kw.size() + size_t(len) > 0x3fffffff) return -1;
    const size_t at = kw.size();
    kw.resize(at + size_t(len), 0);
    return int64_t(at);
  }
  void give_kw(int32_t at, int32_t len) {
    size_t i = 0;
    while (i < kw_free_.size() && kw_free_[i].at < at) ++i;
    kw_free_.insert(kw_free_.begin() + long(i), Range{at, len});
    if (i + 1 < kw_free_.size() && kw_free_[i].at + kw_free_[i].len == kw_free_[i + 1].at) {
      kw_free_[i].len += kw_free_[i + 1].len;
      kw_free_.erase(kw_free_.begin() + long(i) + 1);
    }
    if (i > 0 && kw_free_[i - 1].at + kw_free_[i - 1].len == kw_free_[i].at) {
      kw_free_[i - 1].len += kw_free_[i].len;
      kw_free_.erase(kw_free_.begin() + long(i));
    }
  }
  int32_t take_mask() {
    if (!mask_free_.empty()) {
      size_t lo = 0;
      for (size_t i = 1; i < mask_free_.size(); ++i)
        if (mask_free_[i] < mask_free_[lo]) lo = i;
      const int32_t at = mask_free_[lo];
      mask_free_.erase(mask_free_.begin() + long(lo));
      return at;
    }
    if (mask.size() + size_t(W) > 0x3fffffff) return -1;
    const size_t at = mask.size();
    mask.resize(at + size_t(W), 0u);
    return int32_t(at);
  }
};

}  // namespace wekws
