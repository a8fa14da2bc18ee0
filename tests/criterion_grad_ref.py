"""float64 numpy oracle of the criterion's gradient with respect to its input (wekws_amd.criterion), written
from the closed forms, not from autograd: max-pooling (torch's even split among tied extremes and the inclusive gate of the
clamp), cross entropy (softmax minus one-hot) and CTC (softmax minus the alpha-beta occupancies).  Inputs are the float32
arrays the device gets; everything after them is float64, except the float32 comparisons that decide ties and gates (`1 - x`
is ONE float32 subtraction, as in tests/criterion_ref.py).  Every function returns `g * upstream / divisor`."""
from __future__ import annotations

import numpy as np

_LO, _HI, _ONE = np.float32(1e-8), np.float32(1.0), np.float32(1.0)


def _clamp32(v):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), v, np.minimum(np.maximum(v, _LO), _HI)).astype(np.float32)


def max_pooling_grad(scores, target, lengths, min_duration=0, upstream=1.0, divisor=1):
    """(B, T, K) float64.  A column whose pooled value is NaN (a NaN in one of its unmasked frames) gets zeros: the extreme's
    gradient lands on the NaN frames, and the clamp's gate is false there."""
    s = np.asarray(scores, np.float32)
    B, T, K = s.shape
    lengths = np.clip(np.asarray(lengths, np.int64), 0, T)
    t = np.arange(T)
    g = np.zeros((B, T, K), np.float64)
    for b in range(B):
        pad = t >= lengths[b]
        for j in range(K):
            x = s[b, :, j]
            if int(target[b]) == j:
                masked = pad | (t < min_duration)
                p = _clamp32(np.where(masked, np.float32(0.0), x))
                if np.isnan(p).any():
                    continue
                P = p.max()
                tie = p == P
                with np.errstate(invalid="ignore"):
                    gate = tie & ~masked & (x >= _LO) & (x <= _HI)
                g[b, gate, j] = -(1.0 / np.float64(P)) / int(tie.sum())
            else:
                u = (_ONE - x).astype(np.float32)
                q = _clamp32(np.where(pad, _ONE, u))
                if np.isnan(q).any():
                    continue
                Q = q.min()
                tie = q == Q
                with np.errstate(invalid="ignore"):
                    gate = tie & ~pad & (u >= _LO) & (u <= _HI)
                g[b, gate, j] = (1.0 / np.float64(Q)) / int(tie.sum())
    return g * float(upstream) / divisor


def cross_entropy_grad(logits, target, upstream=1.0, divisor=1):
    """(B, D) float64; a target outside [0, D) or a NaN logit makes the row NaN."""
    x = np.asarray(logits, np.float64)
    B, D = x.shape
    tg = np.asarray(target, np.int64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    g = e / e.sum(axis=1, keepdims=True)
    ok = (tg >= 0) & (tg < D)
    g[np.arange(B)[ok], tg[ok]] -= 1.0
    g[~ok] = np.nan
    return g * float(upstream) / divisor


def _lse_rows(v):
    m = v.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(v - m).sum(axis=-1, keepdims=True)))[..., 0]


def _shift(a, k, left):
    out = np.full_like(a, -np.inf)
    if k < a.size:
        if left:
            out[:a.size - k] = a[k:]
        else:
            out[k:] = a[:a.size - k]
    return out


def _lse3(a, b, c):
    m = np.maximum(np.maximum(a, b), c)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.where(m == -np.inf, -np.inf, ms + np.log(np.exp(a - ms) + np.exp(b - ms) + np.exp(c - ms)))


def ctc_grad(logits, targets, lengths, target_lengths, upstream=1.0, divisor=1):
    """-> dict(grad (B, T, V) f64, rows (B) f64): softmax minus the occupancy of every class's extended states on the valid
    frames, 0 beyond the length; NaN on the valid frames of a row no alignment fits or with a label outside [1, V)."""
    x = np.asarray(logits, np.float64)
    B, T, V = x.shape
    g = np.zeros((B, T, V), np.float64)
    rows = np.empty(B, np.float64)
    for b in range(B):
        n, S = int(np.clip(lengths[b], 0, T)), int(target_lengths[b])
        lab = np.asarray(targets[b][:S], np.int64)
        if ((lab < 1) | (lab >= V)).any():
            rows[b] = np.nan
            g[b, :n] = np.nan
            continue
        if n == 0:
            rows[b] = np.inf if S else 0.0
            continue
        lp = x[b, :n] - _lse_rows(x[b, :n])[:, None]
        ext = np.zeros(2 * S + 1, np.int64)
        ext[1::2] = lab
        L = ext.size
        skip = np.zeros(L, bool)                                # state s may be entered from s - 2
        skip[3::2] = lab[1:] != lab[:-1]
        e = lp[:, ext]                                          # (n, L)
        al = np.full((n, L), -np.inf)
        al[0, 0] = e[0, 0]
        if L > 1:
            al[0, 1] = e[0, 1]
        for t in range(1, n):
            a = al[t - 1]
            al[t] = _lse3(a, _shift(a, 1, False), np.where(skip, _shift(a, 2, False), -np.inf)) + e[t]
        ll = np.logaddexp(al[n - 1, L - 1], al[n - 1, L - 2] if L > 1 else -np.inf)
        rows[b] = -ll
        if not np.isfinite(ll):
            g[b, :n] = np.nan
            continue
        be = np.full((n, L), -np.inf)                           # beta without the frame's own emission
        be[n - 1, L - 1] = 0.0
        if L > 1:
            be[n - 1, L - 2] = 0.0
        skip_out = _shift(skip.astype(np.float64), 2, True) > 0      # state s may leave to s + 2
        for t in range(n - 2, -1, -1):
            f = be[t + 1] + e[t + 1]
            be[t] = _lse3(f, _shift(f, 1, True), np.where(skip_out, _shift(f, 2, True), -np.inf))
        occ = np.exp(al + be - ll)                              # (n, L); every frame's sums to 1
        sm = np.exp(lp)
        for s in range(L):
            sm[:, ext[s]] -= occ[:, s]
        g[b, :n] = sm
    return dict(grad=g * float(upstream) / divisor, rows=rows)
