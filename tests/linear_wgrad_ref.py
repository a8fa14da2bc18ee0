"""The float64 numpy oracle of the Linear weight-gradient tests, and ``emulate``: the arithmetic contract of
wekws_amd/csrc/linear_wgrad_plan.h restated in numpy, operation for operation.

    oracle(x, g)          dw = g^T x and db = sum_r g in float64, and the sums of magnitudes sum_r |g x| and sum_r |g| that the
                          element bound of tests/linear_wgrad_matrix.py is made of
    emulate(x, g, plan)   chains of plan["chain"] rows counted from row 0; per chain the float32 fmaf chain over ascending r from
                          +0; slices of plan["chains_per_slice"] consecutive chains added in double, ascending from +0.0; the
                          slices added in double, ascending from +0.0, and rounded to float32 once.  The bias is the same
                          arithmetic on a column of ones.

A float32 fmaf is computed as the exact double product (24 + 24 significant bits) plus the addend, rounded to double TO ODD and
then to float32: rounding to odd at 53 bits makes the second rounding the correct rounding of the exact sum (Boldo and
Melquiond), which a plain double addition is not when its result falls on a float32 tie.
"""
from __future__ import annotations

import numpy as np


def oracle(x, g):
    """-> dict(dw (O, I), db (O), abs_dw, abs_db) in float64."""
    x64, g64 = np.asarray(x, np.float64), np.asarray(g, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return dict(dw=g64.T @ x64, db=g64.sum(0), abs_dw=np.abs(g64).T @ np.abs(x64), abs_db=np.abs(g64).sum(0))


def fmaf32(a, b, c):
    """float32 fma(a, b, c) of float32 arrays, exactly rounded (see the module's docstring).  Non-finite values go through as
    the double arithmetic has them."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)          # exact
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)                          # TwoSum: s + e == p + c exactly
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        if fix.any():
            s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def plan_of(chain, chains, slices):
    """The plan ``emulate`` needs, from what wekws_hip_linear_wgrad_plan reports: slices are runs of ceil(chains / slices) chains."""
    return dict(chain=int(chain), chains=int(chains), slices=int(slices), chains_per_slice=-(-int(chains) // int(slices)))


def _fold(p, plan):
    """p (chains, ...) float32 chain results -> float32: slices in double ascending, then the fold, rounded once."""
    cps = plan["chains_per_slice"]
    with np.errstate(invalid="ignore", over="ignore"):
        total = np.zeros(p.shape[1:], np.float64)
        for s in range(plan["slices"]):
            part = np.zeros(p.shape[1:], np.float64)
            for c in range(s * cps, min(plan["chains"], (s + 1) * cps)):
                part = part + p[c].astype(np.float64)
            total = total + part
        return total.astype(np.float32)


def emulate(x, g, plan):
    """-> (dw (O, I), db (O)) float32: the bits the device must give."""
    x, g = np.asarray(x, np.float32), np.asarray(g, np.float32)
    R, I = x.shape
    O = g.shape[1]
    K, chains = plan["chain"], plan["chains"]
    assert chains == -(-R // K) and plan["slices"] <= chains
    xp = np.zeros((chains * K, I), np.float32)
    gp = np.zeros((chains * K, O), np.float32)
    xp[:R], gp[:R] = x, g                                         # rows past R: fmaf(0, 0, acc) == acc, acc is never -0
    xp, gp = xp.reshape(chains, K, I), gp.reshape(chains, K, O)
    pw = np.zeros((chains, O, I), np.float32)
    pb = np.zeros((chains, O), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(min(K, R)):
            pw = fmaf32(np.broadcast_to(gp[:, k, :, None], pw.shape), np.broadcast_to(xp[:, k, None, :], pw.shape), pw)
            pb = pb + gp[:, k, :]                                 # float32 addition
    return _fold(pw, plan), _fold(pb, plan)
