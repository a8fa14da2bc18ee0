"""A float64 numpy oracle of a stacked, unidirectional, batch-first GRU (PyTorch's gate order r, z, n) and of its gradients:
the arithmetic of csrc/gru_train.hip.h and the GEMMs around it, as the issue's formulas state them.

    gi = W_ih x + b_ih          gh = W_hh h[t-1] + b_hh
    r = s(gi_r + gh_r)   z = s(gi_z + gh_z)   q = gh_n   n = tanh(gi_n + r q)   h[t] = (1 - z) n + z h[t-1]
    backward, t = T-1 .. 0, dh = grad_y[t] + carry (carry starts at grad_hn):
        dn = dh (1 - z)(1 - n^2)    dz = dh (h[t-1] - n) z (1 - z)    dr = dn q r (1 - r)
        dgi[t] = (dr, dz, dn)       dgh[t] = (dr, dz, dn r)           carry = dh z + W_hh^T dgh[t]
    dW_ih = dgi^T x   dW_hh = dgh^T h_prev   dx = dgi W_ih   db_ih = sum dgi   db_hh = sum dgh   dh0 = the last carry
"""
from __future__ import annotations

import numpy as np


def sigmoid(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(x))
        return np.where(np.isnan(x), np.nan, np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)))


def layer_forward(x, w_ih, w_hh, b_ih, b_hh, h0):
    """x (B, T, I), h0 (B, H) -> (y (B, T, H), saved): everything in float64."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    gi = x @ w_ih.T + b_ih
    y = np.empty((B, T, H))
    r, z, n, q, hp = (np.empty((B, T, H)) for _ in range(5))
    h = h0
    for t in range(T):
        gh = h @ w_hh.T + b_hh
        hp[:, t] = h
        r[:, t] = sigmoid(gi[:, t, :H] + gh[:, :H])
        z[:, t] = sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
        q[:, t] = gh[:, 2 * H:]
        n[:, t] = np.tanh(gi[:, t, 2 * H:] + r[:, t] * q[:, t])
        h = (1.0 - z[:, t]) * n[:, t] + z[:, t] * h
        y[:, t] = h
    return y, dict(x=x, r=r, z=z, n=n, q=q, hp=hp)


def layer_backward(saved, w_ih, w_hh, gy, ghn):
    """gy (B, T, H), ghn (B, H) -> dict(dx, dh0, dw_ih, dw_hh, db_ih, db_hh, dgi, dgh)."""
    x, r, z, n, q, hp = (saved[k] for k in ("x", "r", "z", "n", "q", "hp"))
    B, T, H = r.shape
    dgi, dgh = np.empty((B, T, 3 * H)), np.empty((B, T, 3 * H))
    carry = ghn
    for t in range(T - 1, -1, -1):
        dh = gy[:, t] + carry
        dn = dh * (1.0 - z[:, t]) * (1.0 - n[:, t] ** 2)
        dz = dh * (hp[:, t] - n[:, t]) * z[:, t] * (1.0 - z[:, t])
        dr = dn * q[:, t] * r[:, t] * (1.0 - r[:, t])
        dgi[:, t] = np.concatenate([dr, dz, dn], 1)
        dgh[:, t] = np.concatenate([dr, dz, dn * r[:, t]], 1)
        carry = dh * z[:, t] + dgh[:, t] @ w_hh
    f = lambda a: a.reshape(B * T, -1)  # noqa: E731
    return dict(dx=dgi @ w_ih, dh0=carry, dw_ih=f(dgi).T @ f(x), dw_hh=f(dgh).T @ f(hp), db_ih=f(dgi).sum(0), db_hh=f(dgh).sum(0),
                dgi=dgi, dgh=dgh)


def gru(x, params, h0=None, gy=None, ghn=None):
    """A stack of layers.  params: a list of dicts(w_ih, w_hh, b_ih, b_hh) per layer (biases None: zeros); h0, ghn: (L, B, H) or
    None for zeros; gy (B, T, H) or None for zeros.  -> dict(y, hn, and with gy or ghn: dx, dh0 (L, B, H), and per layer lists
    dw_ih, dw_hh, db_ih, db_hh), float64.  Non-finite values propagate as IEEE arithmetic has them."""
    with np.errstate(all="ignore"):
        x = np.asarray(x, np.float64)
        B, T, _ = x.shape
        L, H = len(params), params[0]["w_hh"].shape[1]
        P = []
        for p in params:
            d = {k: np.asarray(p[k], np.float64) for k in ("w_ih", "w_hh")}
            for k in ("b_ih", "b_hh"):
                d[k] = np.zeros(3 * H) if p.get(k) is None else np.asarray(p[k], np.float64)
            P.append(d)
        h0 = np.zeros((L, B, H)) if h0 is None else np.asarray(h0, np.float64)
        saved, last, inp = [], [], x
        for l in range(L):
            inp, s = layer_forward(inp, P[l]["w_ih"], P[l]["w_hh"], P[l]["b_ih"], P[l]["b_hh"], h0[l])
            saved.append(s)
            last.append(inp[:, -1])
        out = dict(y=inp, hn=np.stack(last))
        if gy is None and ghn is None:
            return out
        g = np.zeros((B, T, H)) if gy is None else np.asarray(gy, np.float64)
        ghn = np.zeros((L, B, H)) if ghn is None else np.asarray(ghn, np.float64)
        grads = [None] * L
        for l in range(L - 1, -1, -1):
            grads[l] = layer_backward(saved[l], P[l]["w_ih"], P[l]["w_hh"], g, ghn[l])
            g = grads[l]["dx"]
        out.update(dx=g, dh0=np.stack([grads[l]["dh0"] for l in range(L)]))
        for k in ("dw_ih", "dw_hh", "db_ih", "db_hh"):
            out[k] = [grads[l][k] for l in range(L)]
        return out

