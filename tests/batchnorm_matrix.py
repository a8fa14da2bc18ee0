"""Case list, units and bars of the BatchNorm1d tests (tests/test_batchnorm_ref.py on the CPU, tests/test_hip_batchnorm.py on the
GPU).  The oracle is tests/batchnorm_ref.py (float64 numpy); the cases named ``g_*`` are also goldens of the live reference's
four sites (tests/golden/batchnorm_golden.npz, made by make_batchnorm_golden.py).

A case is (B, C, T, relu, residual, training, affine, running, momentum, flavour); seeded: x ~ N(0.5, 1.5), g, residual ~ N(0, 1),
weight ~ N(1, 0.3), bias ~ N(0, 0.3), running_mean ~ N(0, 0.5), running_var ~ U(0.5, 1.5), num_batches_tracked = 3, eps = 1e-5.
A training case with running buffers makes two successive calls, the second on the input x2 = 0.5 g + 0.25: y, the saved
statistics and the gradients are the first call's, the running buffers and num_batches_tracked are taken after the second.
R = 8 rows a workgroup, TILE = 128 frames a tile, both from the plan.

    g_*                  the goldens: the reference's sites DsCnnBlock.cnn[1:3] (g_ds), DSDilatedConv1d.bn (g_dsd), TCNBlock.bn1 /
                         relu1 (g_bn1) and bn2 + inputs + relu2 (g_bn2), in train() and in eval() (``_eval``), and bn2's site with a
                         NaN (channel 1), a +Inf (channel 3) and a -Inf (channel 5) in x, in grad_y and in the residual
    r<BC>                B C in 1, 2, R - 1, R, R + 1, 2 R - 1, 2 R, 2 R + 1, 2 R + 2 rows, B = 1 (r1: C = 1)
    t<T>                 T in 1, 2, 3, 4, 5, 6, 7, TILE - 1, TILE, TILE + 1, 2 TILE - 1, 2 TILE, 2 TILE + 1: all four T mod 4
    n2                   B = 2, T = 1: two values a channel
    fold9, fold15, fold20   9, 15 and 20 partials a channel: segments of two with a single last one and of three with a short last
                         one -- both stages of the fold; every case with at most eight partials has one a segment
    f<relu><res><train><affine><running>   the 32 combinations of the flags, shapes cycling through T mod 4
    eval8                the buffers' statistics over rows of a multiple of four frames: the 16-byte instance of that kernel
    mom_0.1, mom_0, mom_1, mom_none        the momentum over two calls (None: the cumulative average over num_batches_tracked)
    off65536, off4096    channels of N(65536, 1) and N(4096, 1): a mean that dwarfs the spread (N = 111 and 800)
    const                a channel of one repeated value: var = 0
    orth, orth_relu      batch rows in pairs with equal x (and residual) and g[odd] = -(1 + 2^-12) g[even]: the gradient sums
                         cancel to 2^-13 of their terms
    recipe_tcn           (256, 64, 100), BN + ReLU: a DsCnnBlock of a ds_tcn.yaml batch
    recipe_mdtc          (100, 32, 200), BN + residual + ReLU: a TCNBlock of an mdtc_small.yaml batch

Units, per element, U = 2^-24:  |got - ref64| / (U sum|terms|), the terms as tests/batchnorm_ref.py lists them; a zero denominator
demands an exact 0; the classes (NaN, +Inf, -Inf) are compared first and exactly, and a non-finite element has no units.  The
backward quantities' reference is the oracle's backward on what a backward call is given: the float32 save_mean and save_invstd
(the device's own; for torch, which keeps its own to itself, the float32 roundings of the oracle's) and, under a ReLU, the
forward's own y, whose zeros are the gate.

BARS -- the project's rule (tests/depthwise_conv_matrix.py): pow2_at_or_above(4 x the worst units of the reference's float32
result against the oracle over this matrix).  The reference's float32 result is torch's CPU ``F.batch_norm`` (+ add, + relu) and
its autograd (tests/test_batchnorm_ref.py recomputes this table; torch does not show its saved statistics, so ``mean`` and
``invstd`` take the float32 ``x.mean`` and ``1 / sqrt(x.var(unbiased=False) + eps)``):

    quantity   reference's worst units   bar    device's worst units (MI355X)
    y          2.80 (t255)               16     2.68 (recipe_tcn)
    mean       2.76 (recipe_tcn)         16     0.80 (r15)
    invstd     1.55 (off4096)            8      0.98 (r15)
    rm         4.74 (r7)                 32     0.93 (orth_relu)
    rv         6.29 (off65536)           32     0.98 (g_nonfinite_res)
    dx         28.37 (off65536)          128    2.50 (recipe_tcn)
    dres       0 (a copy or a zero)      0      0
    dw         6.05 (off65536)           32     0.85 (r16)
    db         1.56 (t2)                 8      1.00 (t4)

Each statistic and parameter gradient of the device is held to a second bound of its own (device_sum_bound): one float32
rounding plus N 2^-53 relative to sum|terms|, which is what double sums and one final rounding can lose.
"""
from __future__ import annotations

import functools
import itertools
import zlib

import numpy as np

from tests import batchnorm_ref as br

U = 2.0 ** -24
EPS = 1e-5
TRACKED0 = 3
QUANTITIES = ("y", "mean", "invstd", "rm", "rv", "dx", "dres", "dw", "db")
SUMS = ("mean", "invstd", "rm", "rv", "dw", "db")                # held to device_sum_bound as well
# measured by tests/test_batchnorm_ref.py (its -s output); dres is a copy or a zero: exact
REF_UNITS = {"y": 2.80, "mean": 2.76, "invstd": 1.55, "rm": 4.74, "rv": 6.29, "dx": 28.37, "dres": 0.0, "dw": 6.05, "db": 1.56}
BARS = {"y": 16.0, "mean": 16.0, "invstd": 8.0, "rm": 32.0, "rv": 32.0, "dx": 128.0, "dres": 0.0, "dw": 32.0, "db": 8.0}  # pow2_at_or_above(4 x)

_SITE = {"ds": (True, False), "dsd": (False, False), "bn1": (True, False), "bn2": (True, True)}   # site -> (relu, residual)
# name -> (B, C, T, relu, residual, training, affine, running, momentum, flavour)
GOLDEN = {
    "g_ds": (3, 5, 7, True, False, True, True, True, 0.1, ""),
    "g_dsd": (2, 4, 9, False, False, True, True, True, 0.1, ""),
    "g_bn1": (2, 3, 5, True, False, True, True, True, 0.1, ""),
    "g_bn2": (2, 6, 11, True, True, True, True, True, 0.1, ""),
    "g_ds_eval": (3, 5, 7, True, False, False, True, True, 0.1, ""),
    "g_dsd_eval": (2, 4, 9, False, False, False, True, True, 0.1, ""),
    "g_bn1_eval": (2, 3, 5, True, False, False, True, True, 0.1, ""),
    "g_bn2_eval": (2, 6, 11, True, True, False, True, True, 0.1, ""),
    "g_nonfinite_x": (2, 6, 10, True, True, True, True, True, 0.1, "nonfinite_x"),
    "g_nonfinite_x_eval": (2, 6, 10, True, True, False, True, True, 0.1, "nonfinite_x"),
    "g_nonfinite_g": (2, 6, 10, True, True, True, True, True, 0.1, "nonfinite_g"),
    "g_nonfinite_res": (2, 6, 10, True, True, True, True, True, 0.1, "nonfinite_res"),
}
GOLDEN_SITE = {"g_ds": "ds", "g_dsd": "dsd", "g_bn1": "bn1", "g_bn2": "bn2", "g_ds_eval": "ds", "g_dsd_eval": "dsd", "g_bn1_eval": "bn1",
               "g_bn2_eval": "bn2", "g_nonfinite_x": "bn2", "g_nonfinite_x_eval": "bn2", "g_nonfinite_g": "bn2", "g_nonfinite_res": "bn2"}


def _cases():
    cases = dict(GOLDEN)
    R, TL = br.ROWS, br.TILE
    for n, BC in enumerate((1, 2, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 2 * R + 2)):
        cases[f"r{BC}"] = (1, BC, 5 + n % 4, n % 2 == 0, n % 3 == 0, True, True, True, 0.1, "")
    for n, T in enumerate((1, 2, 3, 4, 5, 6, 7, TL - 1, TL, TL + 1, 2 * TL - 1, 2 * TL, 2 * TL + 1)):
        cases[f"t{T}"] = (2 + n % 3, (3, 5, 9)[n % 3], T, n % 2 == 1, n % 3 != 1, True, True, True, 0.1, "")
    cases["n2"] = (2, 3, 1, True, True, True, True, True, 0.1, "")
    cases["fold9"] = (3, 5, 2 * TL + 44, True, True, True, True, True, 0.1, "")
    cases["fold15"] = (5, 3, 2 * TL + 3, False, False, True, True, True, 0.1, "")
    cases["fold20"] = (4, 3, 4 * TL + 5, True, False, True, True, True, 0.1, "")
    for n, (relu, res, train, affine, running) in enumerate(itertools.product((False, True), repeat=5)):
        cases["f" + "".join("01"[v] for v in (relu, res, train, affine, running))] = (
            3, 5, 6 + n % 4, relu, res, train, affine, running, 0.1, "")
    cases["eval8"] = (2, 5, 8, True, True, False, True, True, 0.1, "")
    for m in (0.1, 0.0, 1.0, None):
        cases["mom_" + ("none" if m is None else f"{m:g}")] = (3, 4, 9, True, False, True, True, True, m, "")
    cases["off65536"] = (3, 4, 37, True, True, True, True, True, 0.1, "off65536")
    cases["off4096"] = (8, 4, 100, True, False, True, True, True, 0.1, "off4096")
    cases["const"] = (3, 4, 10, True, True, True, True, True, 0.1, "const")
    cases["orth"] = (4, 16, 50, False, True, True, True, True, 0.1, "orth")
    cases["orth_relu"] = (4, 16, 50, True, True, True, True, True, 0.1, "orth")
    cases["recipe_tcn"] = (256, 64, 100, True, False, True, True, True, 0.1, "")
    cases["recipe_mdtc"] = (100, 32, 200, True, True, True, True, True, 0.1, "")
    return cases


CASES = _cases()


def case_names():
    return list(CASES)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


@functools.lru_cache(maxsize=None)
def load_case(name):
    """-> dict(x, g, x2 (B, C, T), res or None, w, b (C) or None, rm, rv (C) or None, tracked (int) or None, float32; relu,
    training, batch_stats, momentum, calls).  Read-only arrays."""
    B, C, T, relu, residual, training, affine, running, momentum, flavour = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = (0.5 + 1.5 * rng.standard_normal((B, C, T))).astype(np.float32)
    g = rng.standard_normal((B, C, T)).astype(np.float32)
    res = rng.standard_normal((B, C, T)).astype(np.float32)
    w = (1.0 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    b = (0.3 * rng.standard_normal(C)).astype(np.float32)
    rm = (0.5 * rng.standard_normal(C)).astype(np.float32)
    rv = (0.5 + rng.random(C)).astype(np.float32)
    if flavour == "nonfinite_x":
        x[0, 1, 3], x[1, 3, 7], x[0, 5, 2] = np.nan, np.inf, -np.inf
    elif flavour == "nonfinite_g":
        g[0, 1, 3], g[1, 3, 7], g[0, 5, 2] = np.nan, np.inf, -np.inf
        res[0, 1, 3], res[1, 3, 7], res[0, 5, 2] = 50.0, 50.0, 50.0        # the ReLU passes there
    elif flavour == "nonfinite_res":
        res[0, 1, 3], res[1, 3, 7], res[0, 5, 2] = np.nan, np.inf, -np.inf
    elif flavour in ("off65536", "off4096"):
        x[:, 1::2] = (float(flavour[3:]) + rng.standard_normal((B, (C + 0) // 2, T))).astype(np.float32)
    elif flavour == "const":
        x[:, 2] = 3.25
    elif flavour == "orth":
        x[1::2], res[1::2] = x[0::2], res[0::2]
        g[1::2] = -(1.0 + 2.0 ** -12) * g[0::2]
    x2 = (0.5 * g + 0.25).astype(np.float32)
    for a in (x, g, x2, res, w, b, rm, rv):
        a.setflags(write=False)
    batch_stats = training or not running
    return dict(x=x, g=g, x2=x2, res=res if residual else None, w=w if affine else None, b=b if affine else None,
                rm=rm if running else None, rv=rv if running else None, tracked=TRACKED0 if running else None, relu=relu,
                training=training, batch_stats=batch_stats, momentum=momentum, calls=2 if training and running else 1)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """-> (ref, mag, tracked): dicts over the forward quantities the case has (y, mean, invstd, rm, rv), float64; the count
    after the calls."""
    c = load_case(name)
    B, _, T = c["x"].shape
    N = B * T
    ref, mag = {}, {}
    tracked = c["tracked"]
    if c["batch_stats"]:
        st, sm = br.batch_stats(c["x"], EPS)
    else:
        st, sm = br.eval_stats(c["rm"], c["rv"], EPS)
    for k in ("mean", "invstd"):
        ref[k], mag[k] = st[k], sm[k]
    ref["y"], mag["y"] = br.forward(c["x"], c["w"], c["b"], c["res"], st["mean"], st["invstd"], c["relu"])
    if c["calls"] == 2:
        rm, rv = c["rm"].astype(np.float64), c["rv"].astype(np.float64)
        for xin in (c["x"], c["x2"]):
            s, _ = br.batch_stats(xin, EPS)
            tracked += 1
            f = br.momentum_factor(c["momentum"], tracked)
            # the buffers are float32 between the calls
            rm, rm_m = br.running_update(f32(rm), s["mean"], f)
            with np.errstate(all="ignore"):
                rv, rv_m = br.running_update(f32(rv), s["var"] * (N / (N - 1.0)), f)
        ref.update(rm=rm, rv=rv)
        mag.update(rm=rm_m, rv=rv_m)
    for a in list(ref.values()) + list(mag.values()):
        a.setflags(write=False)
    return ref, mag, tracked


def backward_oracle(name, y=None, saved=None):
    """-> (ref, mag): dicts over dx, dres (where the case has a residual), dw, db, float64: the oracle's backward on what a
    backward call is given -- the float32 statistics ``saved = (save_mean, save_invstd)`` (None: the float32 roundings of the
    oracle's) and, under a ReLU, the forward's own output ``y`` (None: the oracle's), whose zeros are the ReLU's gate.  A y that
    rounds to the other side of zero is the forward's error and is measured there, not as a gradient that is wholly there or
    wholly gone; the statistics' own errors are measured as ``mean`` and ``invstd``."""
    c = load_case(name)
    ref, _, _ = oracle(name)
    y = ref["y"] if y is None else np.asarray(y, np.float64).reshape(ref["y"].shape)
    mean, invstd = (f32(ref["mean"]), f32(ref["invstd"])) if saved is None else saved
    r, m = br.backward(c["x"], y, c["g"], c["w"], mean, invstd, c["batch_stats"], c["relu"])
    if c["res"] is None:
        del r["dres"], m["dres"]
    return r, m


def same_classes(got, ref):
    """NaN, +Inf and -Inf in the same places."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref))
            and np.array_equal(np.isneginf(got), np.isneginf(ref)))


def worst_units(got, ref, mag):
    """The worst |got - ref| / (U mag) over the elements whose reference is finite; a zero denominator demands an exact 0 (inf
    otherwise), and so does a denominator that is not finite.  The classes are compared by same_classes, first."""
    got, ref, mag = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, mag))
    fin = np.isfinite(ref) & np.isfinite(got)
    err, den = np.abs(got[fin] - ref[fin]), U * mag[fin]
    zero = (den == 0) | ~np.isfinite(den)                           # (an infinite term and a finite result: relu(-Inf) = 0)
    if np.any(err[zero] != 0):
        return float("inf")
    return float((err[~zero] / den[~zero]).max()) if (~zero).any() else 0.0


def units(name, got, saved=None):
    """got: dict over a subset of QUANTITIES -> (dict of worst units, list of quantities whose classes differ).  The gradients
    are held to backward_oracle on got's own y (which a got with gradients of a ReLU case must hold) and on ``saved``."""
    ref, mag, _ = oracle(name)
    if any(k in got for k in ("dx", "dres", "dw", "db")):
        r, m = backward_oracle(name, got["y"] if load_case(name)["relu"] else None, saved)
        ref, mag = {**ref, **r}, {**mag, **m}
    out, bad = {}, []
    for k, v in got.items():
        v = np.asarray(v).reshape(ref[k].shape)
        if not same_classes(v, ref[k]):
            bad.append(k)
        out[k] = worst_units(v, ref[k], mag[k])
    return out, bad


def device_sum_bound(name):
    """The device's own bound on the statistics and the parameter gradients in the units above.  The sums are double sums of
    terms each rounded once in double, so what the device loses is N + 1 roundings of 2^-53 relative to sum|terms| and one final
    rounding to float32: at most 2^-24 of the result, so at most one unit.  The oracle's own float64 sum is allowed as much
    again.  The running buffers are two such calls."""
    B, _, T = CASES[name][:3]
    return 1.0 + 2.0 * 2.0 * (B * T + 1) * 2.0 ** -53 / U
