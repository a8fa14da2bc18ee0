// The per-stream plan of the streaming front end: what one push of n samples does to one stream of
// KeyWordSpotter.accept_wave (wekws/bin/stream_kws_ctc.py:335-398).  Pure host C++, no HIP: this one function decides
// everything the host returns (frames, counts) and everything the kernels are told (stream_frontend.hip.h).
//
// State of a stream:  rem  leftover samples (wave_remained);  fr  remembered feature frames (feature_remained), -1 = none
// yet;  off  the frame-skip phase (feats_ctx_offset).  With L = frame_length, S = frame_shift (samples), l / r the context,
// ds the frame skip, a push of n samples:
//   1. hold      tot = rem + n < L r: keep all tot samples, return None                                   (:348-351)
//   2. fbank     nf snip-edges frames over [rem | chunk]; rem' = tot - nf S                                (:354-364)
//   3. context   assert nf > r; pad = [new[0]] * l + new (first processed chunk) or fr + new; len(pad) - 2 r rows, row i
//                = pad[i : i + l + r + 1]; fr' = new[-(l + r):] -- of the NEW frames only                  (:366-390)
//   4. skip      rows off, off + ds, ... of the k rows; off' = (off - k) mod ds                            (:391-397)
// Context is either off (l = r = 0) or l == r >= 1: the reference raises inside its window loop for l > r and silently
// drops r - l frames per chunk for l < r.
#pragma once
#include <stdint.h>

namespace wekws {

struct StreamFeCfg {
  int32_t frame_length, frame_shift, left, right, skip;
};

struct StreamFeCounts {
  int32_t rem, fr, off;   // fr: -1 = none
};

struct StreamFePlan {
  int32_t status;     // 0, or -1 (WEKWS_HIP_EINVAL) where the reference trips its assertion (:367)
  int32_t held;       // 1: the reference's None; every sample kept, nothing else changes
  int32_t nf;         // fbank frames of this push
  int32_t rem_out;
  int32_t pad_first;  // 1: the rows start with `left` copies of the first new frame
  int32_t fr_in;      // remembered frames in front of the new ones (0 with pad_first)
  int32_t rows_ctx;   // rows after context expansion (nf without context)
  int32_t rows_out;   // rows after the skip: what the caller gets
  int32_t fr_out;
  int32_t off_out;
};
constexpr int kStreamFePlanInts = 10;

// 0 if the configuration is one the front end takes, else -1
inline int stream_fe_cfg_ok(const StreamFeCfg& c) {
  if (c.frame_length <= 0 || c.frame_shift <= 0 || c.frame_shift > c.frame_length) return -1;   // (S > L would skip samples: rem' < 0)
  if (c.left < 0 || c.right < 0 || c.skip < 1) return -1;
  if (c.left != c.right) return -1;
  return 0;
}

// samples a stream may hold between two pushes: rem < max(L, L r)
inline int64_t stream_fe_rem_cap(const StreamFeCfg& c) {
  return int64_t(c.frame_length) * (c.right > 1 ? c.right : 1);
}

// fbank frames that always suffice for a chunk of up to nmax samples, whatever the stream holds
inline int64_t stream_fe_max_nf(const StreamFeCfg& c, int nmax) {
  const int64_t tot = stream_fe_rem_cap(c) - 1 + nmax;
  return tot < c.frame_length ? 0 : 1 + (tot - c.frame_length) / c.frame_shift;
}

// rows that always suffice for a chunk of up to nmax samples: every fresh frame behind the remembered ones (the windows' 2 r
// only take away), every skip-th of them from phase 0
inline int64_t stream_fe_max_rows(const StreamFeCfg& c, int nmax) {
  const int64_t rows = stream_fe_max_nf(c, nmax) + (c.left > 0 ? c.left + c.right : 0);
  return (rows + c.skip - 1) / c.skip;
}

inline StreamFePlan stream_fe_plan(const StreamFeCfg& c, const StreamFeCounts& in, int n) {
  StreamFePlan p{};
  const int64_t L = c.frame_length, S = c.frame_shift;
  const int64_t tot = int64_t(in.rem) + n;
  p.fr_out = in.fr;
  p.off_out = in.off;
  if (tot < L * c.right) {                                   // 1. hold
    p.held = 1;
    p.rem_out = int32_t(tot);
    return p;
  }
  const int64_t nf = tot < L ? 0 : 1 + (tot - L) / S;        // 2. fbank
  p.nf = int32_t(nf);
  p.rem_out = int32_t(tot - nf * S);
  int64_t rows = nf;
  if (c.left > 0) {                                          // 3. context (left == right >= 1)
    if (nf <= c.right) {
      p.status = -1;
      return p;
    }
    p.pad_first = in.fr < 0;
    p.fr_in = in.fr < 0 ? 0 : in.fr;
    rows = (p.pad_first ? c.left : p.fr_in) + nf - 2 * int64_t(c.right);
    if (rows < 0) rows = 0;
    const int64_t keep = int64_t(c.left) + c.right;
    p.fr_out = int32_t(nf < keep ? nf : keep);
  }
  p.rows_ctx = int32_t(rows);
  p.rows_out = p.rows_ctx;
  if (c.skip > 1) {                                          // 4. skip
    p.rows_out = rows > in.off ? int32_t((rows - in.off + c.skip - 1) / c.skip) : 0;
    p.off_out = int32_t(((in.off - rows) % c.skip + c.skip) % c.skip);
  }
  return p;
}

}  // namespace wekws
