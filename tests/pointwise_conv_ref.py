"""The float64 numpy oracle of the pointwise Conv1d tests, and the emulation of the arithmetic contract of
wekws_amd/csrc/pointwise_conv_plan.h in numpy, operation for operation.

    oracle(x, w, bias, g)        y, dx, dw, db in float64 and the sums of magnitudes abs_y = sum_i |w x| + |bias|,
                                 abs_dx = sum_o |w g|, abs_dw = sum_r |g x|, abs_db = sum_r |g| that the element bounds of
                                 tests/pointwise_conv_matrix.py are made of
    emulate_forward(x, w, bias)  acc = +0; i ascending, acc = fmaf(w[o][i], x[b][i][t], acc); then one float32 addition of
                                 bias[o], none without a bias
    emulate_dx(g, w)             the same chain over o ascending, fmaf(w[o][i], g[b][o][t], acc)
    emulate_wgrad(x, g, plan)    tests/linear_wgrad_ref.emulate on the transposed views: rows r = b T + t

x (B, Ci, T), g (B, Co, T), w (Co, Ci), bias (Co) or None.  The float32 fmaf is tests/linear_wgrad_ref.fmaf32.
"""
from __future__ import annotations

import numpy as np

from tests import linear_wgrad_ref as lr


def rows(a):
    """(B, C, T) -> the (B T, C) matrix whose row r = b T + t is a[b][:, t] (a copy)."""
    a = np.asarray(a)
    return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1, a.shape[1])


def oracle(x, w, bias, g):
    """-> dict(y, dx, dw, db, abs_y, abs_dx, abs_dw, abs_db) in float64; db and abs_db are there without a bias too."""
    x64, w64, g64 = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(g, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        y, abs_y = np.matmul(w64, x64), np.matmul(np.abs(w64), np.abs(x64))
        if bias is not None:
            b64 = np.asarray(bias, np.float64)[None, :, None]
            y, abs_y = y + b64, abs_y + np.abs(b64)
        out = dict(y=y, abs_y=abs_y, dx=np.matmul(w64.T, g64), abs_dx=np.matmul(np.abs(w64).T, np.abs(g64)))
        out.update(lr.oracle(rows(x), rows(g)))
    return out


def _chain(w, v):
    """w (M, K), v (B, K, T) float32 -> (B, M, T): the float32 fmaf chain over k ascending from +0."""
    w, v = np.asarray(w, np.float32), np.asarray(v, np.float32)
    B, K, T = v.shape
    acc = np.zeros((B, w.shape[0], T), np.float32)
    for k in range(K):
        acc = lr.fmaf32(np.broadcast_to(w[None, :, k, None], acc.shape), np.broadcast_to(v[:, k, None, :], acc.shape), acc)
    return acc


def emulate_forward(x, w, bias=None):
    """-> y (B, Co, T) float32: the bits the device must give."""
    acc = _chain(w, x)
    if bias is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            acc = acc + np.asarray(bias, np.float32)[None, :, None]            # one float32 addition
    return acc


def emulate_dx(g, w):
    """-> dx (B, Ci, T) float32."""
    return _chain(np.asarray(w, np.float32).T, g)


def emulate_wgrad(x, g, plan):
    """-> (dw (Co, Ci), db (Co)) float32, plan from tests/linear_wgrad_ref.plan_of."""
    return lr.emulate(rows(x), rows(g), plan)
