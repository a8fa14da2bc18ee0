"""Case list, units and bars of the GRU training tests (tests/test_gru_train_ref.py on the CPU, tests/test_hip_gru_train.py on
the GPU).  The oracle is tests/gru_train_ref.py (float64 numpy); ``golden`` is also a golden of the live reference's backbone
(tests/golden/gru_train_golden.npz, made by make_gru_train_golden.py).

Cases (seeded: x, h0, the upstream gradients ~ N(0, 1); parameters ~ U(-1/sqrt(H), 1/sqrt(H)), nn.GRU's default initialisation;
a workgroup owns 16 batch rows and a wave 16 hidden units):

    b<B>             B in 1, 15, 16, 17, 33: inside a tile, the tile's edge, two tiles, a ragged last tile        (T 3, H 16, 1 layer)
    t<T>             T in 1, 2, 3, 7: no recurrence at all, both LDS images, an odd count                         (B 5, H 48, 2 layers)
    h<H>             H in 16, 48, 128: one, three and all eight waves with a unit tile                             (B 17, T 4, 2 layers)
    l<L>             1 to 3 layers; the input size of layer 0 is 20 or 40, never H
    h0_y ... no_hn   with and without h0, under grad_y only, grad_hn only (the other pointer is NULL) and both
    nobias           bias=False
    double           the weights doubled: gates further from 0
    sat              b_ih of +100 on every third and -100 on every sixth entry: s and tanh saturate, nothing is NaN
    nan              a NaN in frame 3 of row 2 of x: that row is NaN from there on, and so is every sum over the batch
    golden           the live reference's init_model backbone (hidden 16, 2 layers), its own initialisation
    recipe           (256, 100, 128) x 2 layers: a batch of examples/hi_xiaowen/s0/conf/gru.yaml

Units, per tensor and case, U = 2^-24:  max|got - ref64| / (U max|ref64|)  over the elements whose reference is finite; a zero
reference tensor demands an exact 0; the classes (NaN, +Inf, -Inf) are compared first and exactly.  A quantity's units are the
worst over the layers.

BARS -- the project's rule (tests/fsmn_memory_matrix.py, tests/batchnorm_matrix.py): pow2_at_or_above(4 x the worst units of
torch's CPU float32 nn.GRU + autograd over this matrix), per quantity; tests/test_gru_train_ref.py recomputes the table:

    quantity   torch's worst units (case)   bar
    y          5.39  (recipe)               32
    hn         7.04  (recipe)               32
    dx         9.08  (double)               64
    dh0        6.08  (double)               32
    dw_ih      8.48  (recipe)               64
    dw_hh      11.31 (recipe)               64
    db_ih      3.79  (double)               16
    db_hh      6.50  (recipe)               32

The negative control: W_hh rounded to float16 at the recipe case must miss the y bar (the oracle itself says by how much:
CONTROL_UNITS).
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import torch
import torch.nn as nn

from tests import gru_train_ref as gr

U = 2.0 ** -24
QUANTITIES = ("y", "hn", "dx", "dh0", "dw_ih", "dw_hh", "db_ih", "db_hh")
# measured by tests/test_gru_train_ref.py::test_bars_are_recomputed (its -s output)
REF_UNITS = {"y": 5.39, "hn": 7.04, "dx": 9.08, "dh0": 6.08, "dw_ih": 8.48, "dw_hh": 11.31, "db_ih": 3.79, "db_hh": 6.50}
BARS = {"y": 32.0, "hn": 32.0, "dx": 64.0, "dh0": 32.0, "dw_ih": 64.0, "dw_hh": 64.0, "db_ih": 16.0, "db_hh": 32.0}      # pow2_at_or_above(4 x REF_UNITS)
CONTROL_UNITS = 1693.2      # y of the recipe case with W_hh rounded to float16, against the oracle: far above BARS["y"]


def _c(B, T, H, L=1, I=20, h0=True, grads="both", bias=True, flavour=""):
    return dict(B=B, T=T, H=H, L=L, I=I, h0=h0, grads=grads, bias=bias, flavour=flavour)


def _cases():
    cases = {}
    for B in (1, 15, 16, 17, 33):
        cases[f"b{B}"] = _c(B, 3, 16)
    for T in (1, 2, 3, 7):
        cases[f"t{T}"] = _c(5, T, 48, L=2, I=40, h0=False)
    for H in (16, 48, 128):
        cases[f"h{H}"] = _c(17, 4, H, L=2)
    for L in (1, 2, 3):
        cases[f"l{L}"] = _c(3, 3, 16, L=L, I=40)
    for h0 in (True, False):
        for grads in ("y", "hn", "both"):
            cases[f"{'h0' if h0 else 'no'}_{grads}"] = _c(4, 5, 16, L=2, h0=h0, grads=grads)
    cases["nobias"] = _c(4, 5, 48, L=2, bias=False)
    cases["double"] = _c(16, 7, 128, L=2, flavour="double")
    cases["sat"] = _c(4, 5, 16, L=2, flavour="sat")
    cases["nan"] = _c(5, 6, 16, L=2, flavour="nan")
    cases["golden"] = _c(3, 5, 16, L=2, I=16, flavour="golden")
    cases["recipe"] = _c(256, 100, 128, L=2, I=128, h0=False)
    return cases


CASES = _cases()
NAN_ROW, NAN_FRAME = 2, 3


def case_names():
    return list(CASES)


def golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gru_train_golden.npz")


@functools.lru_cache(maxsize=None)
def load_case(name):
    """-> dict(spec, x (B, T, I), params [dict(w_ih, w_hh, b_ih, b_hh)], h0, ghn (L, B, H) or None, gy (B, T, H) or None), float32.
    Read-only arrays."""
    s = CASES[name]
    B, T, H, L, I = s["B"], s["T"], s["H"], s["L"], s["I"]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    x, h0, gy, ghn = f(B, T, I), f(L, B, H), f(B, T, H), f(L, B, H)
    k = 1.0 / np.sqrt(H)
    u = lambda *shape: rng.uniform(-k, k, shape).astype(np.float32)  # noqa: E731
    params = [dict(w_ih=u(3 * H, I if l == 0 else H), w_hh=u(3 * H, H), b_ih=u(3 * H), b_hh=u(3 * H)) for l in range(L)]
    if s["flavour"] == "golden":
        g = np.load(golden_path())
        x, h0, gy, ghn = g["x"], g["h0"], g["gy"], g["ghn"]
        params = [{k2: g[f"{k2.replace('w_', 'weight_').replace('b_', 'bias_')}_l{l}"] for k2 in ("w_ih", "w_hh", "b_ih", "b_hh")}
                  for l in range(L)]
    if s["flavour"] == "double":
        for p in params:
            p["w_ih"] *= 2
            p["w_hh"] *= 2
    elif s["flavour"] == "sat":
        for p in params:
            p["b_ih"][0::3] = 100.0
            p["b_ih"][1::6] = -100.0
    elif s["flavour"] == "nan":
        x[NAN_ROW, NAN_FRAME, :] = np.nan
    if not s["bias"]:
        for p in params:
            p["b_ih"] = p["b_hh"] = None
    out = dict(spec=s, x=x, params=params, h0=h0 if s["h0"] else None, gy=gy if s["grads"] in ("y", "both") else None,
               ghn=ghn if s["grads"] in ("hn", "both") else None)
    for a in [x, h0, gy, ghn] + [v for p in params for v in p.values() if v is not None]:
        a.setflags(write=False)
    return out


def quantities(name):
    s = CASES[name]
    return [q for q in QUANTITIES if not (q == "dh0" and not s["h0"]) and not (q in ("db_ih", "db_hh") and not s["bias"])]


@functools.lru_cache(maxsize=None)
def oracle(name):
    """-> dict over quantities(name): a list of float64 tensors each (one a layer for the parameter gradients)."""
    c = load_case(name)
    r = gr.gru(c["x"], c["params"], c["h0"], c["gy"], c["ghn"])
    out = {q: (r[q] if isinstance(r[q], list) else [r[q]]) for q in quantities(name)}
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out


def module(name, cls=nn.GRU, dtype=torch.float32, device="cpu", w_hh_dtype=None):
    """The case's GRU as a ``cls`` module with the case's parameters (w_hh_dtype: W_hh rounded through that dtype first)."""
    c = load_case(name)
    s = c["spec"]
    m = cls(s["I"], s["H"], num_layers=s["L"], bias=s["bias"], batch_first=True)
    with torch.no_grad():
        for l, p in enumerate(c["params"]):
            for k, v in p.items():
                if v is None:
                    continue
                t = torch.from_numpy(v.copy())
                if k == "w_hh" and w_hh_dtype is not None:
                    t = t.to(w_hh_dtype).float()
                getattr(m, f"{k.replace('w_', 'weight_').replace('b_', 'bias_')}_l{l}").copy_(t)
    return m.to(device=device, dtype=dtype)


def run_module(name, m, dtype=torch.float32, device="cpu"):
    """One forward and backward of the case through ``m`` -> dict over quantities(name) of lists of numpy arrays."""
    c = load_case(name)
    t = lambda a: None if a is None else torch.from_numpy(a.copy()).to(device=device, dtype=dtype)  # noqa: E731
    x = t(c["x"]).requires_grad_()
    h0 = t(c["h0"])
    if h0 is not None:
        h0.requires_grad_()
    y, hn = m(x, h0)
    loss = 0
    if c["gy"] is not None:
        loss = loss + (y * t(c["gy"])).sum()
    if c["ghn"] is not None:
        loss = loss + (hn * t(c["ghn"])).sum()
    m.zero_grad()
    loss.backward()
    L = c["spec"]["L"]
    n = lambda a: a.detach().cpu().numpy()  # noqa: E731
    out = dict(y=[n(y)], hn=[n(hn)], dx=[n(x.grad)])
    if h0 is not None:
        out["dh0"] = [n(h0.grad)]
    for q, attr in (("dw_ih", "weight_ih"), ("dw_hh", "weight_hh"), ("db_ih", "bias_ih"), ("db_hh", "bias_hh")):
        if q in quantities(name):
            out[q] = [n(getattr(m, f"{attr}_l{l}").grad) for l in range(L)]
    return out


def same_classes(got, ref):
    """NaN, +Inf and -Inf in the same places."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref))
            and np.array_equal(np.isneginf(got), np.isneginf(ref)))


def tensor_units(got, ref):
    """max|got - ref| / (U max|ref|) over the elements whose reference is finite; a zero reference demands an exact 0 (inf
    otherwise).  The classes are compared by same_classes, first."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    fin = np.isfinite(ref) & np.isfinite(got)
    if not fin.any():
        return 0.0
    err, scale = np.abs(got[fin] - ref[fin]).max(), U * np.abs(ref[fin]).max()
    if scale == 0:
        return 0.0 if err == 0 else float("inf")
    return float(err / scale)


def units(name, got):
    """got: dict over a subset of the quantities -> (dict of worst units over the layers, list of quantities whose classes differ)."""
    ref = oracle(name)
    out, bad = {}, []
    for q, tensors in got.items():
        assert len(tensors) == len(ref[q]), (q, len(tensors), len(ref[q]))
        worst = 0.0
        for a, r in zip(tensors, ref[q]):
            a = np.asarray(a).reshape(r.shape)
            if not same_classes(a, r):
                bad.append(q)
            worst = max(worst, tensor_units(a, r))
        out[q] = worst
    return out, bad
