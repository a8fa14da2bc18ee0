"""CPU oracle for the fused softmax + top-k  --  TEST INFRASTRUCTURE, NOT PRODUCT.

numpy restatement of the first beam prune's numeric part: ``logits.softmax(2)`` (wekws/bin/stream_kws_ctc.py:488)
followed by ``probs.topk(score_beam_size)`` per frame (wekws/model/loss.py:236-238).  Parity status: PINNED --
``tests/golden/make_topk_golden.py`` records torch's ``softmax(-1).topk(k)`` on seeded logits and checks, with the
reference's own ``ctc_prefix_beam_search``, that decoding from ONLY those k values per frame gives the same
hypotheses as decoding from the full posterior matrix; ``tests/test_topk_oracle.py`` checks this file against the
recorded values.
"""
import numpy as np


def softmax_topk(logits, k):
    """(..., K) -> (probs (..., k) float32 descending, index (..., k) int64); equal values: lower index first."""
    x = np.asarray(logits, np.float32)
    m = x.max(axis=-1, keepdims=True)
    e = np.exp((x - m).astype(np.float32)).astype(np.float32)
    p = (e / e.sum(axis=-1, keepdims=True, dtype=np.float32)).astype(np.float32)
    order = np.argsort(-x, axis=-1, kind="stable")[..., :k]
    return np.take_along_axis(p, order, axis=-1), order.astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# The float64 side: what tests/test_hip_softmax_f64.py holds softmax_rows_kernel and softmax_topk_kernel to, class by class.
EPS = 2.0 ** -24                   # half an ulp of 1 in float32: one rounding
TINY = 2.0 ** -126                 # the smallest normal float32


def softmax_f64(logits):
    """(..., K) float32 logits AS GIVEN -> float64 posteriors.  Non-finite logits as torch.softmax has them: a class masked with
    -Inf gets 0; a NaN or +Inf anywhere, or -Inf everywhere, makes the row NaN."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(x - x.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)


def softmax_topk_f64(logits, k):
    """(..., K) -> (float64 probabilities (..., k), index (..., k) int64).  The order is a STABLE order on the logits (descending,
    lower index first): it needs no arithmetic, so an implementation's indices are compared exactly.  Classes masked with -Inf come
    after the finite ones (probability 0, ascending index); a NaN logit is never selected (its row's probabilities are NaN, as
    they are with a +Inf, which ranks first); what is left of the k slots -- K < k, or fewer than k classes that are not NaN --
    is padded with (-1, 0)."""
    x = np.asarray(logits, np.float32)
    K = x.shape[-1]
    p = softmax_f64(x)
    order = np.argsort(-x, axis=-1, kind="stable")                 # (NaN sorts last)
    valid = K - np.isnan(x).sum(axis=-1, keepdims=True)
    idx = np.full(x.shape[:-1] + (k,), -1, np.int64)
    n = min(k, K)
    idx[..., :n] = np.where(np.arange(n) < valid, order[..., :n], -1)
    probs = np.where(idx >= 0, np.take_along_axis(p, np.maximum(idx, 0), axis=-1), 0.0)
    return probs, idx


def softmax_subnormal(logits):
    """The positions whose float64 posterior is positive and below float32's normal range (2^-126)."""
    p = softmax_f64(logits)
    with np.errstate(invalid="ignore"):
        return (p > 0) & (p < TINY)


def softmax_units(got, logits, idx=None):
    """Per element, the error of float32 posteriors `got` against softmax_f64(logits) in the unit
        u = |got - p| / (eps p (1 + (m - l_i))),      eps = 2^-24, p the float64 posterior, m the row's maximum, l_i the logit:
    one rounding of the result, plus the relative error (m - l_i) eps that ONE rounding of the exponent's argument leaves in exp.
    idx (..., k): got holds the posteriors of those classes (top-k: -1 is a padded slot, which must hold 0).
    Classes first: inf wherever got and the oracle are not both finite / both the exact zero of a masked class (or padded slot) /
    both NaN.  A posterior below 2^-126 is not held to the relative bar: 0 <= got <= 2^-125 (flushing to zero is allowed), else
    inf.  (How many such positions a row may have is the matrix's condition, tests/softmax_matrix.py, not this function's.)"""
    x = np.asarray(logits, np.float32).astype(np.float64)
    got = np.asarray(got, np.float32).astype(np.float64)
    p = softmax_f64(logits)
    with np.errstate(all="ignore"):
        d = x.max(axis=-1, keepdims=True) - x
        if idx is not None:
            idx = np.asarray(idx)
            pad = idx < 0
            safe = np.where(pad, 0, idx)
            p = np.where(pad, 0.0, np.take_along_axis(p, safe, axis=-1))
            d = np.where(pad, np.inf, np.take_along_axis(np.broadcast_to(d, x.shape), safe, axis=-1))
        assert got.shape == p.shape, (got.shape, p.shape)
        u = np.full(p.shape, np.inf)
        nan = np.isnan(p)
        u[nan & np.isnan(got)] = 0.0
        zero = ~nan & (p == 0.0) & np.isposinf(d)                  # masked classes of a row that has finite ones, padded slots
        u[zero & (got == 0.0)] = 0.0
        sub = ~nan & ~zero & (p < TINY)
        u[sub & (got >= 0.0) & (got <= 2.0 * TINY)] = 0.0
        fin = ~nan & ~zero & ~sub & np.isfinite(got)
        u[fin] = (np.abs(got - p) / (EPS * p * (1.0 + d)))[fin]
    return u
