"""Case list, units and bars of the optimiser-step tests (tests/test_optim_ref.py on the CPU, tests/test_hip_optim.py on the
GPU).  No goldens: the reference -- torch's clip_grad_norm_ + optim.Adam in float32 on the CPU -- exists on every machine.

Scenarios (hyper-parameters of the recipes: lr 1e-3, betas (0.9, 0.999), eps 1e-8, weight_decay 1e-4, grad_clip 5, unless
stated; seeded; no gradient in the float32 subnormals):

    first_clip     the first step from zero moments, a gradient of norm ~20: clipping active
    first_noclip   the first step from zero moments, a gradient of norm ~1: coef is exactly 1
    s1000_noclip   the step after 999, plain Adam.step(): max_norm = +Inf
    s12345_clip    the step after 12,344 with clipping, weight_decay 5e-5, and every 97th element a very small v (1e-14) beside
                   a large m (0.1 .. 0.3): updates far larger than lr
    tiny_grad      gradients of 1e-9 on parameters of 1e-5, moments to match: eps dominates sqrt(v)
    zero7          every 7th gradient exactly 0
    cancel         moments opposite to the gradient: m = -(1 - beta1) / beta1 * g to the last bits, so m' cancels
    wd0            weight_decay = 0

Lengths: 1, 3, 4, 5, 63, 64, 65 (whole float4s and the scalar tail), one tile minus 1, one tile, one tile plus 1, two tiles plus
3, 256 tiles plus 5 (257 partials: the fold's second stage), 300,000 (a DS-TCN's size).  first_clip and s12345_clip run at every
length, every scenario at 65, two tiles plus 3 and 300,000.

Units, per element, U = 2^-24, c the oracle's coefficient, ga = c |g| + wd |p|:

    norm   |d| / (U norm64)
    m'     |d| / (U (beta1 |m| + (1 - beta1) ga))
    v'     |d| / (U (beta2 v + (1 - beta2) ga^2))
    p'     |d| / (U (|p| + |p'64 - p|))

and a zero denominator demands an exact 0.  The denominators are the magnitudes of the terms, not of the results: c g + wd p and
beta1 m + (1 - beta1) g~ cancel.  The scale of p' includes the update's own size: a small v beside a large m makes an update
far larger than lr.

BARS -- the project's rule (tests/criterion_matrix.py): pow2_at_or_above(4 x the worst units of the reference's float32 step
against the float64 oracle, tests/optim_ref.py, over this matrix); recomputed and asserted by tests/test_optim_ref.py:

    quantity   reference's worst units            bar      device's worst units (MI355X)
    norm       681.05  (first_clip_n1048581)      4096     0.76   (s1000_noclip_n300000)
    m          683.04  (first_clip_n1048581)      4096     3.75   (s12345_clip_n300000)
    v          1366.35 (first_clip_n1048581)      8192     7.12   (s12345_clip_n1048581)
    p          4288.43 (first_clip_n1048581)      32768    312.19 (cancel_n300000; the reference: 240.51 there)

The reference's figures are its norm's: torch's CPU float32 sum of squares is 105 units off at 300,000 elements and 681 at
1,048,581, and with clipping active the coefficient carries that error into every element.  tests/test_hip_optim.py therefore
holds the device to a second set of bounds as well, derived from its own arithmetic (DEVICE_BOUND there).
"""
from __future__ import annotations

import functools
import math
import zlib

import numpy as np

from tests import optim_ref

U = 2.0 ** -24
TILE = optim_ref.TILE_FLOATS
LENGTHS = (1, 3, 4, 5, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, optim_ref.FOLD_SEG * TILE + 5, 300000)
SCENARIOS = ("first_clip", "first_noclip", "s1000_noclip", "s12345_clip", "tiny_grad", "zero7", "cancel", "wd0")
REF_UNITS = {"norm": 681.05, "m": 683.04, "v": 1366.35, "p": 4288.43}            # measured by tests/test_optim_ref.py (its -s output)
BARS = {"norm": 4096.0, "m": 4096.0, "v": 8192.0, "p": 32768.0}              # pow2_at_or_above(4 x REF_UNITS)


def case_names():
    names = [f"{s}_n{n}" for s in ("first_clip", "s12345_clip") for n in LENGTHS]
    names += [f"{s}_n{n}" for s in SCENARIOS for n in (65, 2 * TILE + 3, 300000) if f"{s}_n{n}" not in names]
    return names


@functools.lru_cache(maxsize=None)
def load_case(name):
    """-> dict(p, g, m, v float32 (n); step; hyper = dict(lr, betas, eps, weight_decay, max_norm)).  Read-only arrays."""
    scen, n = name.rsplit("_n", 1)
    n = int(n)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, max_norm=5.0)
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    g = (rng.standard_normal(n) / math.sqrt(n)).astype(np.float32)                 # norm ~1
    m = np.zeros(n, np.float32)
    v = np.zeros(n, np.float32)
    step = 0
    if scen == "first_clip":
        g = (20.0 * rng.standard_normal(n) / math.sqrt(n)).astype(np.float32)
        g[0] = np.float32(math.copysign(max(abs(float(g[0])), 20.0), float(g[0]) or 1.0))   # (n = 1, 3, ...: above the clip for certain)
    elif scen == "first_noclip":
        pass
    else:
        m = (0.3 * g * rng.uniform(0.5, 1.5, n) + 0.1 / math.sqrt(n) * rng.standard_normal(n)).astype(np.float32)
        v = ((g.astype(np.float64) * rng.uniform(0.5, 1.5, n)) ** 2 + 1e-3 / n).astype(np.float32)
        if scen == "s1000_noclip":
            step, hyper["max_norm"] = 999, math.inf
        elif scen == "s12345_clip":
            step, hyper["weight_decay"] = 12344, 5e-5
            g = (g * np.float32(20.0)).astype(np.float32)
            g[0] = np.float32(math.copysign(max(abs(float(g[0])), 20.0), float(g[0]) or 1.0))
            v = (v * np.float32(400.0)).astype(np.float32)
            m[::97] = (rng.uniform(0.1, 0.3, len(m[::97])) * rng.choice([-1.0, 1.0], len(m[::97]))).astype(np.float32)
            v[::97] = np.float32(1e-14)
        elif scen == "tiny_grad":
            step = 50
            p = (1e-5 * rng.standard_normal(n)).astype(np.float32)
            g = (1e-9 * rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
            m = (0.5 * g * rng.uniform(0.5, 1.5, n)).astype(np.float32)
            v = ((g.astype(np.float64) * rng.uniform(0.5, 1.5, n)) ** 2).astype(np.float32)
        elif scen == "zero7":
            step = 10
            g[::7] = 0.0
        elif scen == "cancel":
            step = 200
            m = (-(1.0 - 0.9) / 0.9 * g.astype(np.float64)).astype(np.float32)
        elif scen == "wd0":
            step, hyper["weight_decay"] = 5, 0.0
        else:
            raise KeyError(name)
    assert not np.any((g != 0) & (np.abs(g) < np.finfo(np.float32).tiny))
    for a in (p, g, m, v):
        a.setflags(write=False)
    return dict(p=p, g=g, m=m, v=v, step=step, hyper=hyper)


@functools.lru_cache(maxsize=None)
def oracle(name):
    c = load_case(name)
    return optim_ref.oracle_step(c["p"], c["g"], c["m"], c["v"], c["step"], **c["hyper"])


def _worst(err, den):
    """max err / den with a zero denominator demanding an exact 0; inf for anything not finite."""
    if not np.all(np.isfinite(err)):
        return float("inf")
    zero = den == 0
    if np.any(err[zero] != 0):
        return float("inf")
    ok = ~zero
    return float((err[ok] / den[ok]).max()) if ok.any() else 0.0


def units(case, ref, got):
    """Worst error of got = dict(norm, p, m, v) against the oracle's ref, in the units of the bars: dict(norm, m, v, p)."""
    p, g, m, v = (np.asarray(case[k], np.float64) for k in ("p", "g", "m", "v"))
    beta1, beta2 = case["hyper"]["betas"]
    ga = ref["coef"] * np.abs(g) + case["hyper"]["weight_decay"] * np.abs(p)
    d = {k: np.abs(np.asarray(got[k], np.float64) - ref[k]) for k in ("norm", "p", "m", "v")}
    return dict(norm=_worst(np.atleast_1d(d["norm"]), np.atleast_1d(U * ref["norm"])),
                m=_worst(d["m"], U * (beta1 * np.abs(m) + (1.0 - beta1) * ga)),
                v=_worst(d["v"], U * (beta2 * v + (1.0 - beta2) * ga * ga)),
                p=_worst(d["p"], U * (np.abs(p) + np.abs(ref["p"] - p))))
