"""The float64 numpy oracle of the dense Conv1d tests, and the emulation of the arithmetic contract of
wekws_amd/csrc/dense_conv_plan.h in numpy, operation for operation.

    oracle(x, w, bias, g, d, P)        y, dx, dw, db in float64 and the sums of magnitudes abs_y = sum_{k,i} |w xp| + |bias|,
                                       abs_dx = sum_{k,o} |w g|, abs_dw = sum_r |g xp|, abs_db = sum_r |g| that the element bounds
                                       of tests/dense_conv_matrix.py are made of
    emulate_forward(x, w, bias, d, P)  acc = +0; k ascending and, inside it, i ascending,
                                       acc = fmaf(w[o][i][k], xp[b][i][t + k d - P], acc); then one float32 addition of bias[o],
                                       none without a bias.  The padding's zeros are operands.
    emulate_dx(g, w, d, P, Tin)        the same chain over k ascending and, inside it, o ascending,
                                       fmaf(w[o][i][k], g[b][o][n + P - k d], acc), g a zero outside [0, Tout)
    emulate_wgrad(x, g, d, P, K, plan) tests/linear_wgrad_ref.emulate tap by tap on the shifted rows: rows r = b Tout + t

x (B, Ci, Tin), g (B, Co, Tout), w (Co, Ci, K), bias (Co) or None, Tout = Tin + P - (K - 1) d.  The float32 fmaf is
tests/linear_wgrad_ref.fmaf32.
"""
from __future__ import annotations

import numpy as np

from tests import linear_wgrad_ref as lr
from tests.pointwise_conv_ref import rows


def tout(Tin, K, d, P):
    return Tin + P - (K - 1) * d


def shifted(a, shift, n):
    """a (B, C, T) -> (B, C, n): column j is a[:, :, j + shift], a zero where j + shift is outside [0, T)."""
    a = np.asarray(a)
    T = a.shape[2]
    out = np.zeros(a.shape[:2] + (n,), a.dtype)
    lo, hi = max(0, -shift), min(n, T - shift)
    if hi > lo:
        out[:, :, lo:hi] = a[:, :, lo + shift:hi + shift]
    return out


def oracle(x, w, bias, g, d, P):
    """-> dict(y, dx, dw, db, abs_y, abs_dx, abs_dw, abs_db) in float64; db and abs_db are there without a bias too."""
    x64, w64, g64 = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(g, np.float64)
    B, Ci, Tin = x64.shape
    Co, _, K = w64.shape
    To = tout(Tin, K, d, P)
    assert g64.shape == (B, Co, To)
    y, abs_y = np.zeros((B, Co, To)), np.zeros((B, Co, To))
    dx, abs_dx = np.zeros((B, Ci, Tin)), np.zeros((B, Ci, Tin))
    dw, abs_dw = np.zeros((Co, Ci, K)), np.zeros((Co, Ci, K))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            xs = shifted(x64, k * d - P, To)
            gs = shifted(g64, P - k * d, Tin)
            y, abs_y = y + np.matmul(w64[:, :, k], xs), abs_y + np.matmul(np.abs(w64[:, :, k]), np.abs(xs))
            dx, abs_dx = dx + np.matmul(w64[:, :, k].T, gs), abs_dx + np.matmul(np.abs(w64[:, :, k]).T, np.abs(gs))
            o = lr.oracle(rows(xs), rows(g64))
            dw[:, :, k], abs_dw[:, :, k] = o["dw"], o["abs_dw"]
        if bias is not None:
            b64 = np.asarray(bias, np.float64)[None, :, None]
            y, abs_y = y + b64, abs_y + np.abs(b64)
        return dict(y=y, abs_y=abs_y, dx=dx, abs_dx=abs_dx, dw=dw, abs_dw=abs_dw, db=o["db"], abs_db=o["abs_db"])


def _chain(w, v, shifts, n):
    """w (M, C, K), v (B, C, T) float32 -> (B, M, n): the float32 fmaf chain over k ascending and, inside it, c ascending, from
    +0, of w[m][c][k] v[b][c][j + shifts[k]]."""
    w, v = np.asarray(w, np.float32), np.asarray(v, np.float32)
    acc = np.zeros((v.shape[0], w.shape[0], n), np.float32)
    for k, shift in enumerate(shifts):
        vs = shifted(v, shift, n)
        for c in range(w.shape[1]):
            acc = lr.fmaf32(np.broadcast_to(w[None, :, c, k, None], acc.shape), np.broadcast_to(vs[:, c, None, :], acc.shape), acc)
    return acc


def emulate_forward(x, w, bias, d, P):
    """-> y (B, Co, Tout) float32: the bits the device must give."""
    K = np.asarray(w).shape[2]
    acc = _chain(w, x, [k * d - P for k in range(K)], tout(np.asarray(x).shape[2], K, d, P))
    if bias is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            acc = acc + np.asarray(bias, np.float32)[None, :, None]            # one float32 addition
    return acc


def emulate_dx(g, w, d, P, Tin):
    """-> dx (B, Ci, Tin) float32."""
    K = np.asarray(w).shape[2]
    return _chain(np.asarray(w, np.float32).transpose(1, 0, 2), g, [P - k * d for k in range(K)], Tin)


def emulate_wgrad(x, g, d, P, K, plan):
    """-> (dw (Co, Ci, K), db (Co)) float32, plan from tests/linear_wgrad_ref.plan_of."""
    x, g = np.asarray(x, np.float32), np.asarray(g, np.float32)
    To = g.shape[2]
    gr = rows(g)
    dw = np.zeros((g.shape[1], x.shape[1], K), np.float32)
    db = None
    for k in range(K):
        dw[:, :, k], b = lr.emulate(rows(shifted(x, k * d - P, To)), gr, plan)
        db = b if db is None else db
    return dw, db
