"""float64 oracle of the trainable BatchNorm1d with its fused ReLU and residual add (csrc/batchnorm.hip.h, include/wekws_hip.h):
every formula of the header comment in numpy, each quantity together with the sum of the absolute values of its terms, which is
what the tests' units are relative to; and the plan of csrc/batchnorm_plan.h restated (tiles, fold, workspace).

    x, y, residual, g: (B, C, T);  N = B T;  per channel
    mean = sum x / N                               terms x / N
    var = sum (x - mean)^2 / N                     terms (x - mean)^2 / N          (all of one sign: the sum of terms is var)
    invstd = 1 / sqrt(var + eps)                   one term
    z = x a - mean a + bias + residual, a = invstd weight      four terms;  y = relu(z) keeps z's terms
    running <- (1 - f) running + f new             two terms
    g' = g where not (y <= 0)                      (a NaN y passes the gradient, as torch's threshold_backward does)
    db = sum g'                                    terms g'
    dw = invstd sum g' (x - mean)                  terms invstd g' (x - mean)
    dx = a (g' - db / N - (x - mean) invstd^2 S / N),  S = sum g' (x - mean):
                                                   |a| (|g'| + sum|g'| / N + |x - mean| invstd^2 sum|g' (x - mean)| / N)
    dx = a g'  (statistics from the running buffers)            one term
"""
from __future__ import annotations

import numpy as np

ROWS = 8                # (b, c) rows a workgroup                    (csrc/batchnorm_plan.h)
TILE = 128              # frames of a row a workgroup owns: one partial each
FOLD_SEGS = 8
FOLD_CHANS = 32


def tiles_t(T):
    return (T + TILE - 1) // TILE


def partials(B, T):
    return B * tiles_t(T)


def fold_seg_len(n):
    return (n + FOLD_SEGS - 1) // FOLD_SEGS


def check(B, C, T):
    if min(B, C, T) < 1 or max(B, C, T) > 2**31 - 1:
        return False
    return (B * C + ROWS - 1) // ROWS * tiles_t(T) <= 2**31 - 1


def workspace_bytes(B, C, T):
    """(partials, C, 2) doubles, (C, 2) floats, 16 bytes; each part rounded up to 16."""
    if not check(B, C, T):
        return 0
    up = lambda n: (n + 15) // 16 * 16  # noqa: E731
    return up(partials(B, T) * C * 2 * 8) + up(C * 2 * 4) + 16


def _bc(v, ndim=3):
    """(C) -> (1, C, 1)"""
    return np.asarray(v, np.float64).reshape((1, -1) + (1,) * (ndim - 2))


def batch_stats(x, eps):
    """-> (ref, mag): dicts over mean, var, invstd (C), float64."""
    x = np.asarray(x, np.float64)
    N = x.shape[0] * x.shape[2]
    with np.errstate(all="ignore"):
        mean = x.sum(axis=(0, 2)) / N
        dev2 = (x - _bc(mean)) ** 2
        var = dev2.sum(axis=(0, 2)) / N
        invstd = 1.0 / np.sqrt(var + eps)
        mags = {"mean": np.abs(x).sum(axis=(0, 2)) / N, "var": var.copy(), "invstd": np.abs(invstd)}
    return {"mean": mean, "var": var, "invstd": invstd}, mags


def eval_stats(running_mean, running_var, eps):
    rm, rv = np.asarray(running_mean, np.float64), np.asarray(running_var, np.float64)
    with np.errstate(all="ignore"):
        invstd = 1.0 / np.sqrt(rv + eps)
    return {"mean": rm.copy(), "invstd": invstd}, {"mean": np.abs(rm), "invstd": np.abs(invstd)}


def forward(x, weight, bias, residual, mean, invstd, relu):
    """-> (y, mag) (B, C, T) float64.  weight / bias / residual None: absent."""
    x = np.asarray(x, np.float64)
    C = x.shape[1]
    w = np.ones(C) if weight is None else np.asarray(weight, np.float64)
    b = np.zeros(C) if bias is None else np.asarray(bias, np.float64)
    with np.errstate(all="ignore"):
        a = _bc(np.asarray(invstd, np.float64) * w)
        z = (x - _bc(mean)) * a + _bc(b)
        mag = np.abs(x * a) + np.abs(_bc(mean) * a) + np.abs(_bc(b))
        if residual is not None:
            r = np.asarray(residual, np.float64)
            z = z + r
            mag = mag + np.abs(r)
        if relu:
            z = np.where(z < 0, 0.0, z)                              # a NaN stays a NaN
    return z, mag


def running_update(running, new, f):
    """(1 - f) running + f new -> (value, mag)."""
    running, new = np.asarray(running, np.float64), np.asarray(new, np.float64)
    with np.errstate(all="ignore"):
        return (1.0 - f) * running + f * new, np.abs((1.0 - f) * running) + np.abs(f * new)


def momentum_factor(momentum, tracked_after):
    return 1.0 / tracked_after if momentum is None else momentum


def backward(x, y, g, weight, mean, invstd, use_batch_stats, relu):
    """mean, invstd: the saved statistics the backward call is given.  -> (ref, mag): dicts over dx, dres (B, C, T), dw, db (C)."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    C = x.shape[1]
    N = x.shape[0] * x.shape[2]
    w = np.ones(C) if weight is None else np.asarray(weight, np.float64)
    mean, invstd = np.asarray(mean, np.float64), np.asarray(invstd, np.float64)
    with np.errstate(all="ignore"):
        gp = np.where(np.asarray(y, np.float64) <= 0, 0.0, g) if relu else g.copy()
        d = x - _bc(mean)
        db, db_m = gp.sum(axis=(0, 2)), np.abs(gp).sum(axis=(0, 2))
        S, S_m = (gp * d).sum(axis=(0, 2)), np.abs(gp * d).sum(axis=(0, 2))
        dw, dw_m = invstd * S, np.abs(invstd) * S_m
        a = _bc(invstd * w)
        if use_batch_stats:
            dx = a * (gp - _bc(db) / N - d * _bc(invstd ** 2 * S) / N)
            dx_m = np.abs(a) * (np.abs(gp) + _bc(db_m) / N + np.abs(d) * _bc(invstd ** 2 * S_m) / N)
        else:
            dx, dx_m = a * gp, np.abs(a * gp)
    return {"dx": dx, "dres": gp, "dw": dw, "db": db}, {"dx": dx_m, "dres": np.abs(gp), "dw": dw_m, "db": db_m}
