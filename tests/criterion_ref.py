"""float64 numpy oracle of the validation criterion (wekws_amd.criterion), written from the formulas, not from the
reference's source: the three losses, the pooled values, the correctness flags, the edit distance and the utterance accuracy.
Inputs are the float32 arrays the device gets; everything after them is float64 (except `1 - p`, which the definition
takes as ONE float32 subtraction, and the pooled values, which are float32 by comparisons alone)."""
from __future__ import annotations

import numpy as np

from tests import ctc_kws_ref


def _nanmax(v):
    return np.float32(np.nan) if np.isnan(v).any() else v.max()


def _nanmin(v):
    return np.float32(np.nan) if np.isnan(v).any() else v.min()


def max_pooling(scores, target, lengths, min_duration=0):
    """-> dict(pooled (B, K) f32, terms (B, K) f64, loss f64, correct (B) int32, acc float)."""
    s = np.asarray(scores, np.float32)
    B, T, K = s.shape
    lengths = np.clip(np.asarray(lengths, np.int64), 0, T)
    pooled = np.empty((B, K), np.float32)
    correct = np.zeros(B, np.int32)
    t = np.arange(T)
    lo, hi, one = np.float32(1e-8), np.float32(1.0), np.float32(1.0)
    for b in range(B):
        pad = t >= lengths[b]
        for j in range(K):
            p = s[b, :, j]
            if int(target[b]) == j:
                v = np.where(pad | (t < min_duration), np.float32(0.0), p)
                with np.errstate(invalid="ignore"):
                    v = np.where(np.isnan(v), v, np.minimum(np.maximum(v, lo), hi))
                pooled[b, j] = _nanmax(v)
            else:
                v = np.where(pad, one, (one - p).astype(np.float32))
                with np.errstate(invalid="ignore"):
                    v = np.where(np.isnan(v), v, np.minimum(np.maximum(v, lo), hi))
                pooled[b, j] = _nanmin(v)
        m = np.array([_nanmax(np.where(pad, np.float32(0.0), s[b, :, j])) for j in range(K)], np.float32)
        if np.isnan(m).any():
            continue                                       # a NaN is neither > 0.5 nor < 0.5
        idx = int(np.argmax(m))                            # first maximum
        if (m[idx] > 0.5 and idx == int(target[b])) or (m[idx] < 0.5 and int(target[b]) < 0):
            correct[b] = 1
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = -np.log(pooled.astype(np.float64))
    return dict(pooled=pooled, terms=terms, loss=terms.sum() / B, correct=correct, acc=int(correct.sum()) / B)


def _lse(v, axis=-1):
    v = np.asarray(v, np.float64)
    m = v.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(v - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def cross_entropy(logits, target):
    """-> dict(rows (B) f64, loss, pred (B) int32, correct (B) int32, acc)."""
    x = np.asarray(logits, np.float64)
    B, D = x.shape
    tg = np.asarray(target, np.int64)
    ok = (tg >= 0) & (tg < D)
    rows = np.where(ok, _lse(x) - x[np.arange(B), np.clip(tg, 0, D - 1)], np.nan)
    pred = np.argmax(np.asarray(logits, np.float32), axis=1).astype(np.int32)
    correct = (ok & (pred == tg)).astype(np.int32)
    return dict(rows=rows, loss=rows.sum() / B, pred=pred, correct=correct, acc=int(correct.sum()) * 100.0 / B)


def _logaddexp3(a, b, c):
    m = max(a, b, c)
    if m == -np.inf:
        return -np.inf
    return m + np.log(np.exp(a - m) + np.exp(b - m) + np.exp(c - m))


def ctc(logits, targets, lengths, target_lengths, skip_equal_labels=False):
    """-log p(labels | logits) per row by the alpha recursion over blank-extended labels; +Inf where no alignment fits.
    skip_equal_labels=True is the WRONG recursion (the skip transition between equal labels too): the negative control."""
    x = np.asarray(logits, np.float64)
    B, T, V = x.shape
    rows = np.empty(B, np.float64)
    for b in range(B):
        n, S = int(np.clip(lengths[b], 0, T)), int(target_lengths[b])
        lab = [int(v) for v in targets[b][:S]]
        if any(c < 1 or c >= V for c in lab):
            rows[b] = np.nan
            continue
        if n == 0:
            rows[b] = np.inf if S else 0.0
            continue
        lp = x[b, :n] - _lse(x[b, :n])[:, None]
        ext = [0]
        for c in lab:
            ext += [c, 0]
        L = len(ext)
        a = np.full(L, -np.inf)
        a[0] = lp[0, 0]
        if L > 1:
            a[1] = lp[0, ext[1]]
        for t in range(1, n):
            na = np.full(L, -np.inf)
            for s in range(L):
                skip = s >= 2 and ext[s] != 0 and (skip_equal_labels or ext[s] != ext[s - 2])
                na[s] = _logaddexp3(a[s], a[s - 1] if s >= 1 else -np.inf, a[s - 2] if skip else -np.inf) + lp[t, ext[s]]
            a = na
        rows[b] = -_logaddexp3(a[L - 1], a[L - 2] if L > 1 else -np.inf, -np.inf)
    return dict(rows=rows, loss=rows.sum() / B)


def edit_distance(lab, rec):
    lab, rec = list(lab), list(rec)
    d = list(range(len(rec) + 1))
    for i in range(1, len(lab) + 1):
        prev, d[0] = d[0], i
        for j in range(1, len(rec) + 1):
            cur = min(d[j] + 1, d[j - 1] + 1, prev + (lab[i - 1] != rec[j - 1]))
            prev, d[j] = d[j], cur
    return d[len(rec)]


def softmax32(logits):
    x = np.asarray(logits, np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def utterance_accuracy(logits, targets, lengths, target_lengths):
    """acc_utterance: prefix beam search (no token set, beams 3 / 5) on the float32 posteriors, the first hypothesis
    against the labels.  -> dict(dist (B) int32, words, errors, acc) ; acc raises ZeroDivisionError without a label."""
    probs = softmax32(logits)
    B, T, _ = probs.shape
    dist = np.zeros(B, np.int32)
    words = errors = 0
    for b in range(B):
        beam, _ = ctc_kws_ref.prefix_beam_search(probs[b, :int(np.clip(lengths[b], 0, T))], 3, 5, None)
        hyp = list(beam[0].prefix) if beam else []
        lab = [int(v) for v in targets[b][:int(target_lengths[b])]]
        dist[b] = edit_distance(lab, hyp)
        if lab:
            words += len(lab)
            errors += int(dist[b])
    return dict(dist=dist, words=words, errors=errors, acc=float(words - errors) * 100.0 / words)


def executor_loop(batches):
    """The host loop of Executor.cv over recorded (loss float32, acc float, num_utts): the statement-by-statement restatement."""
    num_seen_utts, total_loss, total_acc = 1, 0.0, 0.0
    for loss, acc, num_utts in batches:
        if np.isfinite(loss):
            num_seen_utts += num_utts
            total_loss += float(loss) * num_utts
            total_acc += acc * num_utts
    return total_loss / num_seen_utts, total_acc / num_seen_utts
