"""Float64 numpy oracle of the trainable FSMN memory block (wekws_amd/csrc/fsmn_memory.hip.h) and the kernels' plan restated
(wekws_amd/csrc/fsmn_memory_plan.h).  With R = rorder * rstride and x[b, n, d] = 0 for n < 0:

    y[b,t,d]  = x[b,t-R,d] + sum_i wl[d,i] x[b, t-R-(lorder-1-i) lstride, d] + sum_j wr[d,j] x[b, t-R+(j+1) rstride, d]
    dx[b,n,d] = sum over the same taps (coefficient c_k, delay d_k >= 0) of c_k g[b, n+d_k, d]    (n + d_k < T only)
    dwl[d,i]  = sum_{b,t} g[b,t,d] x[b, t-R-(lorder-1-i) lstride, d]
    dwr[d,j]  = sum_{b,t} g[b,t,d] x[b, t-R+(j+1) rstride, d]

Every function also returns the sum of the magnitudes of its terms: the denominators of the tests' units.  The zeros before
frame 0 are arithmetic zeros in y, dwl and dwr (the reference multiplies into its padding); terms past the end of dx do not exist.
"""
from __future__ import annotations

import numpy as np

# ---- the plan (fsmn_memory_plan.h)
MAX_TAPS = 32
MAX_WINDOW = 256
CHANNELS = 32
FIR_TILE = 64
GRAD_TILE = 128
FOLD_SEGS = 8
SKIP, LEFT, RIGHT = 0, 1, 2


def taps(lorder, rorder, lstride, rstride):
    """[(source, index, delay)] in the order the products are added."""
    R = rorder * rstride
    return ([(SKIP, 0, R)] + [(LEFT, i, R + (lorder - 1 - i) * lstride) for i in range(lorder)]
            + [(RIGHT, j, R - (j + 1) * rstride) for j in range(rorder)])


def window(lorder, rorder, lstride, rstride):
    return rorder * rstride + (lorder - 1) * lstride + 1


def check(B, T, D, lorder, rorder, lstride=1, rstride=1):
    """True where the calls accept the shape."""
    return (min(B, T, D) >= 1 and lorder >= 1 and rorder >= 1 and lstride >= 1 and rstride >= 1 and lorder + rorder <= MAX_TAPS
            and window(lorder, rorder, lstride, rstride) <= MAX_WINDOW)


def grad_tiles(B, T):
    return B * ((T + GRAD_TILE - 1) // GRAD_TILE)


def fold_seg_len(tiles):
    return (tiles + FOLD_SEGS - 1) // FOLD_SEGS


def workspace_bytes(B, T, D, lorder, rorder):
    return (grad_tiles(B, T) * (lorder + rorder) * D * 8 + 15) // 16 * 16


# ---- the arithmetic
def _coef(tap, wl, wr):
    s, i, _ = tap
    if s == SKIP:
        return np.ones(wl.shape[0], np.float64)
    return np.asarray(wl if s == LEFT else wr, np.float64)[:, i]


def _delayed(x, d):
    """x[b, t - d, :] with zeros before frame 0, float64."""
    x = np.asarray(x, np.float64)
    out = np.zeros_like(x)
    if d < x.shape[1]:
        out[:, d:] = x[:, :x.shape[1] - d]
    return out


def forward(x, wl, wr, lstride=1, rstride=1):
    """-> (y, sum|terms|), float64 (B, T, D)."""
    wl, wr = np.asarray(wl).reshape(x.shape[2], -1), np.asarray(wr).reshape(x.shape[2], -1)
    y = np.zeros(x.shape, np.float64)
    mag = np.zeros(x.shape, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for tap in taps(wl.shape[1], wr.shape[1], lstride, rstride):
            term = _coef(tap, wl, wr)[None, None, :] * _delayed(x, tap[2])
            y += term
            mag += np.abs(term)
    return y, mag


def backward(x, g, wl, wr, lstride=1, rstride=1):
    """-> dict(dx, dwl, dwr) and dict of the same keys with sum|terms|; dwl (D, lorder), dwr (D, rorder)."""
    D, T = x.shape[2], x.shape[1]
    wl, wr = np.asarray(wl).reshape(D, -1), np.asarray(wr).reshape(D, -1)
    g64 = np.asarray(g, np.float64)
    dx, dxm = np.zeros(x.shape, np.float64), np.zeros(x.shape, np.float64)
    dw = {LEFT: np.zeros(wl.shape, np.float64), RIGHT: np.zeros(wr.shape, np.float64)}
    dwm = {LEFT: np.zeros(wl.shape, np.float64), RIGHT: np.zeros(wr.shape, np.float64)}
    with np.errstate(invalid="ignore", over="ignore"):
        for tap in taps(wl.shape[1], wr.shape[1], lstride, rstride):
            s, i, d = tap
            if d < T:                                  # dx[n] += c g[n + d] for n + d < T: terms past the end do not exist
                term = _coef(tap, wl, wr)[None, None, :] * g64[:, d:]
                dx[:, :T - d] += term
                dxm[:, :T - d] += np.abs(term)
            if s != SKIP:
                prod = g64 * _delayed(x, d)            # the padding's zeros are multiplied: an Inf in g makes a NaN, as in the reference
                dw[s][:, i] = prod.sum(axis=(0, 1))
                dwm[s][:, i] = np.abs(prod).sum(axis=(0, 1))
    return dict(dx=dx, dwl=dw[LEFT], dwr=dw[RIGHT]), dict(dx=dxm, dwl=dwm[LEFT], dwr=dwm[RIGHT])
