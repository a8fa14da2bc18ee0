"""float64 restatement of torchaudio.transforms.Resample(orig, new) with its defaults (sinc_interp_hann,
lowpass_filter_width 6, rolloff 0.99) -- the `resample` step of wekws/dataset/processor.py:83-103 -- and of the streaming
plan of wekws_amd/csrc/resample_plan.h.  numpy and Python integers only; independent of the library.

    g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) rolloff, width = ceil(lpw o / base), K = 2 width + o
    t[i][m]    = clamp(((m - width) / o - i / n) base, -lpw, +lpw)
    k[i][m]    = float32(sinc(pi t) cos^2(pi t / (2 lpw)) base / o)
    y[j n + i] = sum_m k[i][m] x[j o + m - width],   len(y) = ceil(n L / o)
"""
import math

import numpy as np

PAIRS = ((48000, 16000), (8000, 16000), (44100, 16000), (24000, 16000))       # n = 1; o = 1; 160 phases; o = 3, n = 2


class Plan:
    def __init__(self, orig, new, lpw=6, rolloff=0.99):
        g = math.gcd(orig, new)
        self.orig, self.new, self.lpw = orig, new, lpw
        self.o, self.n = orig // g, new // g
        if orig == new:
            self.width, self.K = 0, 1
            self.t = np.zeros((1, 1))
            self.taps64 = np.ones((1, 1))
            self.live = np.ones((1, 1), dtype=bool)
        else:
            o, n = self.o, self.n
            self.base = min(o, n) * rolloff
            self.width = int(math.ceil(lpw * o / self.base))
            self.K = 2 * self.width + o
            idx = np.arange(-self.width, self.width + o, dtype=np.float64)[None, :] / o
            t = (np.arange(0, -n, -1, dtype=np.float64)[:, None] / n + idx) * self.base
            self.live = np.abs(t) < lpw                       # the clamp is inactive
            t = np.clip(t, -lpw, lpw)
            window = np.cos(t * math.pi / lpw / 2) ** 2
            t = t * math.pi
            scale = self.base / o
            with np.errstate(invalid="ignore", divide="ignore"):
                k = np.where(t == 0, 1.0, np.sin(t) / t)
            self.taps64 = k * (window * scale)
        self.taps = self.taps64.astype(np.float32)            # what the reference's convolution is given
        self.first = self.live.argmax(axis=1)
        self.last = self.K - 1 - self.live[:, ::-1].argmax(axis=1)
        assert all(self.live[i, self.first[i]:self.last[i] + 1].all() and self.live[i].sum() == self.last[i] - self.first[i] + 1
                   for i in range(self.n))

    def num_samples(self, L):
        return -((-self.n * int(L)) // self.o)                # Python integers: exact at any length

    # ---- streaming: an output is emitted once every live tap of it lies on a received sample
    def need(self, q):
        j, i = divmod(int(q), self.n)
        return j * self.o + int(self.last[i]) - self.width + 1

    def lo(self, q):
        j, i = divmod(int(q), self.n)
        return j * self.o + int(self.first[i]) - self.width

    def emit_count(self, N):
        """outputs whose live taps all lie in [.., N): counted phase by phase, no bisection, no monotonicity assumed"""
        tot = 0
        for i in range(self.n):
            top = N - 1 - int(self.last[i]) + self.width      # j o <= top
            if top >= 0:
                tot += top // self.o + 1
        return tot

    def step(self, N, nsamp, flush):
        N2 = N + nsamp
        if flush:
            return self.num_samples(N2), N2
        total = self.emit_count(N2)
        return total, min(max(self.lo(total), 0), N2)

    def lookahead_bound(self):
        """received samples at or past the position q o / n of the first output not yet emitted: ceil(lpw o / base) + 1"""
        return self.width + 1


def resample(plan, x, full=False):
    """y (float64) and the bar's sum |k| |x| per output, with the float32 taps.  ``full``: all K taps (what the reference
    convolves; decides NaN / Inf classes), else the live ones (identical for finite input)."""
    x = np.asarray(x, dtype=np.float64)
    L = x.size
    cnt = plan.num_samples(L)
    nblk = -(-cnt // plan.n) if cnt else 0
    pad = np.concatenate([np.zeros(plan.width), x, np.zeros(plan.width + plan.o + nblk * plan.o)])
    if nblk == 0:
        return np.zeros(0), np.zeros(0)
    win = np.lib.stride_tricks.sliding_window_view(pad, plan.K)[::plan.o][:nblk]          # (nblk, K)
    k = plan.taps.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if full:
            y = np.einsum("jm,im->ji", win, k)
            mag = np.einsum("jm,im->ji", np.abs(win), np.abs(k))
        else:
            kl = np.where(plan.live, k, 0.0)
            wz = np.where(np.isfinite(win), win, 0.0)
            y = np.einsum("jm,im->ji", wz, kl)
            mag = np.einsum("jm,im->ji", np.abs(wz), np.abs(kl))
    return y.reshape(-1)[:cnt], mag.reshape(-1)[:cnt]


def classes(plan, x):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf per output of the FULL-window convolution in float32 terms: a term k x with k == 0 and x
    non-finite is NaN; otherwise signs of infinities decide."""
    x = np.asarray(x, dtype=np.float32)
    L = x.size
    cnt = plan.num_samples(L)
    nblk = -(-cnt // plan.n) if cnt else 0
    pad = np.concatenate([np.zeros(plan.width, np.float32), x, np.zeros(plan.width + plan.o + nblk * plan.o, np.float32)])
    out = np.zeros(cnt, dtype=np.int64)
    bad = np.flatnonzero(~np.isfinite(pad))
    for q in range(cnt):
        j, i = divmod(q, plan.n)
        a = j * plan.o
        hit = bad[(bad >= a) & (bad < a + plan.K)]
        if hit.size == 0:
            continue
        with np.errstate(invalid="ignore"):
            terms = plan.taps[i, hit - a] * pad[hit]
        if np.isnan(terms).any() or (np.isposinf(terms).any() and np.isneginf(terms).any()):
            out[q] = 1
        elif np.isposinf(terms).any():
            out[q] = 2
        elif np.isneginf(terms).any():
            out[q] = 3
    return out


def classify(y):
    y = np.asarray(y)
    return np.where(np.isnan(y), 1, np.where(np.isposinf(y), 2, np.where(np.isneginf(y), 3, 0)))


def bar(plan, mag):
    """(live_i + 2) 2^-24 sum_m |k[i][m]| |x|: the forward error bound of a live_i-term float32 accumulation plus one rounding of
    each tap"""
    live = (plan.last - plan.first + 1).astype(np.float64)
    i = np.arange(mag.size) % plan.n
    return (live[i] + 2.0) * 2.0 ** -24 * mag


def to_i16(y):
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)
