"""Float64 numpy oracle of the trainable depthwise Conv1d (wekws_amd/csrc/depthwise_conv.hip.h) and the kernels' plan restated
(wekws_amd/csrc/depthwise_conv_plan.h).  x (B, C, Tin), w (C, K), bias (C) or None, dilation d, left_pad P; with
Tout = Tin + P - (K-1) d and xp[b, c, n] = 0 for n < 0:

    y[b,c,t]  = bias[c] + sum_k w[c,k] xp[b,c, t + k d - P]
    dx[b,c,n] = sum_k w[c,k] g[b,c, n + P - k d]              (terms with an index outside [0, Tout) do not exist)
    dw[c,k]   = sum_{b,t} g[b,c,t] xp[b,c, t + k d - P]
    db[c]     = sum_{b,t} g[b,c,t]

Every function also returns the sum of the magnitudes of its terms (the bias counted as a term of y): the denominators of the
tests' units.  The zeros in front of a row are arithmetic zeros in y and dw (the reference multiplies into its padding).
"""
from __future__ import annotations

import numpy as np

# ---- the plan (depthwise_conv_plan.h)
MAX_TAPS = 32
MAX_WINDOW = 256
ROWS = 8                 # R: (b, c) rows a workgroup owns
FIR_TILE = 128           # FT
GRAD_TILE = 128          # GT
FOLD_SEGS = 8
FOLD_COLS = 32
LEFT = 1


def taps(K, d):
    """[(source, index, delay)] in the order the products are added: fsmn_memory_plan.h's left taps, delays counted back from
    the last tap."""
    return [(LEFT, k, (K - 1 - k) * d) for k in range(K)]


def window(K, d):
    return (K - 1) * d + 1


def tout(Tin, K, d, P):
    return Tin + P - (K - 1) * d


def check(B, C, Tin, K, d, P):
    """True where the calls accept the shape."""
    return bool(min(B, C, Tin) >= 1 and 1 <= K <= MAX_TAPS and d >= 1 and window(K, d) <= MAX_WINDOW and 0 <= P <= (K - 1) * d
                and tout(Tin, K, d, P) >= 1 and max(B, C, Tin) < 2 ** 31
                and -(-B * C // ROWS) * -(-Tin // FIR_TILE) < 2 ** 31)


def grad_tiles(B, C, Tout):
    """Workgroups of the tap-gradient kernel."""
    return -(-B * C // ROWS) * -(-Tout // GRAD_TILE)


def partials(B, Tout):
    """Partial sums a (channel, tap) pair has: what the fold adds."""
    return B * -(-Tout // GRAD_TILE)


def fold_seg_len(n):
    return (n + FOLD_SEGS - 1) // FOLD_SEGS


def workspace_bytes(B, C, Tin, K, d, P):
    return (partials(B, tout(Tin, K, d, P)) * C * (K + 1) * 8 + 15) // 16 * 16


def stage_stride(tile, win):
    return (tile + win - 1 + 3 + 3) // 4 * 4


def fir_lds_bytes(win):
    return ROWS * (stage_stride(FIR_TILE, win) + FIR_TILE + MAX_TAPS + 1) * 4


def grad_lds_bytes(win):
    return ROWS * (stage_stride(GRAD_TILE, win) + GRAD_TILE) * 4


# ---- the arithmetic
def _padded(x, P):
    x = np.asarray(x, np.float64)
    return np.concatenate([np.zeros(x.shape[:2] + (P,), np.float64), x], axis=2)


def forward(x, w, bias, d, P):
    """-> (y, sum|terms|), float64 (B, C, Tout)."""
    B, C, Tin = x.shape
    w = np.asarray(w, np.float64).reshape(C, -1)
    K = w.shape[1]
    To = tout(Tin, K, d, P)
    xp = _padded(x, P)
    y = np.zeros((B, C, To), np.float64)
    mag = np.zeros((B, C, To), np.float64)
    if bias is not None:
        b = np.asarray(bias, np.float64)[None, :, None]
        y += b
        mag += np.abs(b)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            term = w[None, :, k, None] * xp[:, :, k * d:k * d + To]
            y += term
            mag += np.abs(term)
    return y, mag


def backward(x, g, w, d, P):
    """-> dict(dx, dw, db) and dict of the same keys with sum|terms|; dx (B, C, Tin), dw (C, K), db (C)."""
    B, C, Tin = x.shape
    w = np.asarray(w, np.float64).reshape(C, -1)
    K = w.shape[1]
    To = tout(Tin, K, d, P)
    g64 = np.asarray(g, np.float64)
    assert g64.shape == (B, C, To)
    xp = _padded(x, P)
    dxp, dxpm = np.zeros(xp.shape, np.float64), np.zeros(xp.shape, np.float64)
    dw, dwm = np.zeros((C, K), np.float64), np.zeros((C, K), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            term = w[None, :, k, None] * g64                      # dx[n] += w[k] g[n + P - k d]: only terms that exist
            dxp[:, :, k * d:k * d + To] += term
            dxpm[:, :, k * d:k * d + To] += np.abs(term)
            prod = g64 * xp[:, :, k * d:k * d + To]               # the padding's zeros are multiplied
            dw[:, k] = prod.sum(axis=(0, 2))
            dwm[:, k] = np.abs(prod).sum(axis=(0, 2))
    return (dict(dx=dxp[:, :, P:], dw=dw, db=g64.sum(axis=(0, 2))),
            dict(dx=dxpm[:, :, P:], dw=dwm, db=np.abs(g64).sum(axis=(0, 2))))
