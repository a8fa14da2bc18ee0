"""Case list, units and bars of the FSMN memory-block tests (tests/test_fsmn_memory_ref.py on the CPU,
tests/test_hip_fsmn_memory.py on the GPU).  The oracle is tests/fsmn_memory_ref.py (float64 numpy); the cases named ``g_*`` are
also goldens of the live reference's FSMNBlock (tests/golden/fsmn_memory_golden.npz, made by make_fsmn_memory_golden.py).

Cases (seeded: x, g ~ N(0, 1), taps ~ N(0, 0.3); window = rorder rstride + (lorder - 1) lstride + 1; the FIR kernel's tile is 64
frames, the tap gradient's 128):

    g_t1 ... g_inf_tap   the goldens: T shorter than every delay but one, small and odd shapes, strides 2 and 3, a NaN and an Inf
                         frame in x, an Inf tap (forward only)
    d<D>                 D in 1, 3, 4, 5, 64, 128, 130, 250 (16-byte accesses for D % 4 == 0, scalars otherwise; one, four and
                         eight channel blocks, a ragged last one)
    t<T>_<taps>          for each tap set -- (10,2,1,1), (4,3,2,3), (1,1,1,1), (3,1,1,1), (20,12,1,1) -- T in 1, 2, window - 1,
                         window, window + 1, and for (10,2,1,1) also 63, 64, 65, 131 (the FIR tile) and 127, 128, 129, 259 (the
                         tap gradient's tile); B cycles through 1..5
    fold9, fold15        9 and 15 tiles of the tap gradient: segments of two tiles, the last one short (9) or single (15) -- both
                         stages of the fold; every smaller case has one tile a segment
    orth                 rows in pairs with equal x and g[odd] = -(1 + 2^-12) g[even]: the tap sums cancel to 2^-13 of their terms
    recipe               (256, 100, 128) with (10,2,1,1): a batch of examples/hi_xiaowen/s0/conf/fsmn_ctc.yaml

Units, per element, U = 2^-24:  |got - ref64| / (U sum|terms|)  for y, dx, dwl and dwr alike; a zero denominator demands an
exact 0; the classes (NaN, +Inf, -Inf) are compared first and exactly, and a non-finite element has no units.

BARS -- the project's rule (tests/criterion_matrix.py, tests/optim_matrix.py): pow2_at_or_above(4 x the worst units of the
reference's float32 result against the oracle over this matrix).  The reference's float32 result is FSMNBlock's torch path on the
CPU, which restates the reference statement by statement and equals the live reference's golden y bit for bit
(tests/test_fsmn_memory_ref.py, which also recomputes this table):

    quantity   reference's worst units   bar    device's worst units (MI355X)
    y          4.20 (recipe)             32     5.47 (recipe)
    dx         3.99 (recipe)             16     5.11 (recipe)
    dwl        3.05 (g_mid)              16     0.97 (t15_s)
    dwr        2.93 (d250)               16     0.92 (g_l3r1)

The device's tap gradients are held to a second bound of their own (device_dw_bound): one float32 rounding plus N 2^-53 relative
to sum|terms|, N = B T, which is what a double accumulation of exact products and one final rounding can lose.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

from tests import fsmn_memory_ref as fr

U = 2.0 ** -24
QUANTITIES = ("y", "dx", "dwl", "dwr")
REF_UNITS = {"y": 4.20, "dx": 3.99, "dwl": 3.05, "dwr": 2.93}        # measured by tests/test_fsmn_memory_ref.py (its -s output)
BARS = {"y": 32.0, "dx": 16.0, "dwl": 16.0, "dwr": 16.0}          # pow2_at_or_above(4 x REF_UNITS)

RECIPE_TAPS = (10, 2, 1, 1)
TAP_SETS = {"r": RECIPE_TAPS, "s": (4, 3, 2, 3), "one": (1, 1, 1, 1), "l3": (3, 1, 1, 1), "long": (20, 12, 1, 1)}

# name -> (B, T, D, (lorder, rorder, lstride, rstride), flavour)
GOLDEN = {
    "g_t1": (2, 1, 3, RECIPE_TAPS, ""),
    "g_small": (3, 5, 8, RECIPE_TAPS, ""),
    "g_mid": (2, 37, 128, RECIPE_TAPS, ""),
    "g_stride": (2, 40, 20, (4, 3, 2, 3), ""),
    "g_l3r1": (1, 3, 5, (3, 1, 1, 1), ""),
    "g_nonfinite_x": (2, 20, 8, RECIPE_TAPS, "nonfinite_x"),
    "g_inf_tap": (2, 9, 4, RECIPE_TAPS, "inf_tap"),
}
FORWARD_ONLY = ("g_inf_tap",)


def _cases():
    cases = dict(GOLDEN)
    for D in (1, 3, 4, 5, 64, 128, 130, 250):
        cases[f"d{D}"] = (2, 20, D, RECIPE_TAPS, "")
    n = 0
    for key, taps in TAP_SETS.items():
        w = fr.window(*taps)
        ts = [1, 2, w - 1, w, w + 1]
        if key == "r":
            ts += [fr.FIR_TILE - 1, fr.FIR_TILE, fr.FIR_TILE + 1, 2 * fr.FIR_TILE + 3, fr.GRAD_TILE - 1, fr.GRAD_TILE, fr.GRAD_TILE + 1,
                   2 * fr.GRAD_TILE + 3]
        for T in sorted(set(t for t in ts if t >= 1)):
            cases[f"t{T}_{key}"] = (1 + n % 5, T, (8, 5, 12, 6, 36)[n % 5], taps, "")
            n += 1
    cases["fold9"] = (3, 2 * fr.GRAD_TILE + 44, 8, RECIPE_TAPS, "")
    cases["fold15"] = (5, 2 * fr.GRAD_TILE + 3, 6, RECIPE_TAPS, "")
    cases["orth"] = (4, 50, 16, RECIPE_TAPS, "orth")
    cases["recipe"] = (256, 100, 128, RECIPE_TAPS, "")
    return cases


CASES = _cases()


def case_names():
    return list(CASES)


@functools.lru_cache(maxsize=None)
def load_case(name):
    """-> dict(x, g (B, T, D), wl (D, lorder), wr (D, rorder) float32; lstride, rstride; backward: bool).  Read-only arrays."""
    B, T, D, (lorder, rorder, lstride, rstride), flavour = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    g = rng.standard_normal((B, T, D)).astype(np.float32)
    wl = (0.3 * rng.standard_normal((D, lorder))).astype(np.float32)
    wr = (0.3 * rng.standard_normal((D, rorder))).astype(np.float32)
    if flavour == "nonfinite_x":
        x[0, 3, :] = np.nan
        x[1, 11, :] = np.inf
        x[1, 12, ::2] = -np.inf
    elif flavour == "inf_tap":
        wl[1, lorder - 1] = np.inf
        wr[2, 0] = -np.inf
    elif flavour == "orth":
        x[1::2] = x[0::2]
        g[1::2] = -(1.0 + 2.0 ** -12) * g[0::2]
    for a in (x, g, wl, wr):
        a.setflags(write=False)
    return dict(x=x, g=g, wl=wl, wr=wr, lstride=lstride, rstride=rstride, backward=name not in FORWARD_ONLY)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """-> (ref, mag): dicts over y, dx, dwl, dwr (dx, dwl, dwr only where the case runs backward), float64."""
    c = load_case(name)
    y, ym = fr.forward(c["x"], c["wl"], c["wr"], c["lstride"], c["rstride"])
    ref, mag = {"y": y}, {"y": ym}
    if c["backward"]:
        r, m = fr.backward(c["x"], c["g"], c["wl"], c["wr"], c["lstride"], c["rstride"])
        ref.update(r)
        mag.update(m)
    for a in list(ref.values()) + list(mag.values()):
        a.setflags(write=False)
    return ref, mag


def same_classes(got, ref):
    """NaN, +Inf and -Inf in the same places."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref))
            and np.array_equal(np.isneginf(got), np.isneginf(ref)))


def worst_units(got, ref, mag):
    """The worst |got - ref| / (U mag) over the elements whose reference is finite; a zero denominator demands an exact 0 (inf
    otherwise).  The classes are compared by same_classes, first."""
    got, ref, mag = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, mag))
    fin = np.isfinite(ref) & np.isfinite(got)
    err, den = np.abs(got[fin] - ref[fin]), U * mag[fin]
    zero = den == 0
    if np.any(err[zero] != 0) or not np.all(np.isfinite(den)):
        return float("inf")
    return float((err[~zero] / den[~zero]).max()) if (~zero).any() else 0.0


def units(name, got):
    """got: dict over a subset of y, dx, dwl, dwr -> (dict of worst units, list of quantities whose classes differ)."""
    ref, mag = oracle(name)
    out, bad = {}, []
    for k, v in got.items():
        v = np.asarray(v).reshape(ref[k].shape)
        if not same_classes(v, ref[k]):
            bad.append(k)
        out[k] = worst_units(v, ref[k], mag[k])
    return out, bad


def device_dw_bound(name):
    """The device's own bound on dwl and dwr in the units above.  The products of two floats are exact in double and the sums are
    double, so what the device loses is N roundings of 2^-53 relative to sum|terms| (N = B T terms a tap) and one final rounding
    to float32: at most 2^-24 of the result, so at most one unit.  The oracle's own float64 sum is allowed as much again."""
    B, T = CASES[name][:2]
    return 1.0 + 2.0 * B * T * 2.0 ** -53 / U
