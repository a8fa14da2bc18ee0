"""Case list, units and bars of the depthwise Conv1d tests (tests/test_depthwise_conv_ref.py on the CPU,
tests/test_hip_depthwise_conv.py on the GPU).  The oracle is tests/depthwise_conv_ref.py (float64 numpy); the cases named
``g_*`` are also goldens of the live reference's depthwise convolutions (tests/golden/depthwise_conv_golden.npz, made by
make_depthwise_conv_golden.py).

Cases (seeded: x, g ~ N(0, 1), taps and bias ~ N(0, 0.3); window = (K-1) d + 1; R = 8 rows a workgroup, FT = GT = 128 frames
a tile, all from the plan):

    g_t1 ... g_inf_tap   the goldens: Tout = 1, Tin shorter than the window with P making up the rest, small odd shapes,
                         (K, d) in (8,1), (8,8), (5,4), (3,2), (1,1), with and without bias, a NaN and an Inf sample in x, an
                         Inf tap under P > 0 (forward only)
    c<C>                 C in 1, 3, 4, 5, R-1, R, R+1, 64, 66 with B = 1: rows short of, equal to and past a workgroup's
    p<P>_<taps>          P in 0, 1, (K-1) d - 1, (K-1) d for (8,8) and (5,4)
    t<Tout>_<taps>       for each (K, d), full padding: Tout in 1, 2, window - 1, window, window + 1, and for (8,8) also
                         FT - 1, FT, FT + 1, 2 FT + 3 (the tiles of the FIR and of the tap-gradient kernel); B cycles through 1..5
    len<a><b>            Tin = a and Tout = b (mod 4) for a, b in 0..3: the 16-byte instance (a = b = 0) and the scalar one
    fold9, fold15, fold20   9, 15 and 20 partials a (channel, tap) pair: segments of two with a single last one (9: five
                         segments; 15: eight) and of three with a short last one (20) -- both stages of the fold; every case with
                         at most eight partials has one a segment
    orth                 batch rows in pairs with equal x and g[odd] = -(1 + 2^-12) g[even]: dw and db cancel to 2^-13 of their terms
    recipe_tcn           (256, 64, 100), K = 8, d = 8, P = 56: the deepest block of a ds_tcn.yaml batch
    recipe_mdtc          (100, 32, 200), K = 5, d = 8, P = 32: the deepest block of an mdtc_small.yaml batch
    long                 K = 32, d = 8: the longest window the plan takes, 249 frames

Units, per element, U = 2^-24:  |got - ref64| / (U sum|terms|)  for y, dx, dw and db alike (the bias is a term of y); a zero
denominator demands an exact 0; the classes (NaN, +Inf, -Inf) are compared first and exactly, and a non-finite element has no
units.

BARS -- the project's rule (tests/fsmn_memory_matrix.py): pow2_at_or_above(4 x the worst units of the reference's float32 result
against the oracle over this matrix).  The reference's float32 result is torch's CPU ``F.conv1d(F.pad(x, (P, 0)), ...,
groups=C)``, which equals the live reference's golden y bit for bit (tests/test_depthwise_conv_ref.py, which also recomputes
this table):

    quantity   reference's worst units   bar    device's worst units (MI355X)
    y          3.78 (recipe_tcn)         16     3.78 (recipe_tcn)
    dx         4.02 (recipe_tcn)         32     4.02 (recipe_tcn)
    dw         1.94 (t7_k8d1)            8      0.94 (t7_k8d1)
    db         0.97 (g_t1)               4      0.97 (g_t1)

The device's dw and db are held to a second bound of their own (device_dw_bound): one float32 rounding plus N 2^-53 relative to
sum|terms|, N = B Tout, which is what a double accumulation of exact products and one final rounding can lose.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

from tests import depthwise_conv_ref as dr

U = 2.0 ** -24
QUANTITIES = ("y", "dx", "dw", "db")
REF_UNITS = {"y": 3.78, "dx": 4.02, "dw": 1.94, "db": 0.97}         # measured by tests/test_depthwise_conv_ref.py (its -s output)
BARS = {"y": 16.0, "dx": 32.0, "dw": 8.0, "db": 4.0}             # pow2_at_or_above(4 x REF_UNITS)

TAP_SETS = {"k8d1": (8, 1), "k8d8": (8, 8), "k5d4": (5, 4), "k3d2": (3, 2), "k1d1": (1, 1)}

# name -> (B, C, Tin, K, d, P, bias, flavour)
GOLDEN = {
    "g_t1": (2, 3, 8, 8, 1, 0, True, ""),                         # Tout = 1
    "g_short": (2, 3, 20, 8, 8, 56, True, ""),                    # Tin shorter than the window of 57
    "g_small": (3, 5, 7, 5, 4, 16, False, ""),
    "g_k3": (1, 3, 9, 3, 2, 2, False, ""),                        # half the padding
    "g_k1": (2, 2, 5, 1, 1, 0, True, ""),
    "g_mid": (2, 8, 37, 8, 1, 7, True, ""),
    "g_nonfinite_x": (2, 4, 20, 5, 4, 16, True, "nonfinite_x"),
    "g_inf_tap": (2, 4, 9, 8, 1, 7, False, "inf_tap"),
}
FORWARD_ONLY = ("g_inf_tap",)


def _cases():
    cases = dict(GOLDEN)
    for C in (1, 3, 4, 5, dr.ROWS - 1, dr.ROWS, dr.ROWS + 1, 64, 66):
        cases[f"c{C}"] = (1, C, 20, 5, 4, 16, C % 2 == 1, "")
    for key in ("k8d8", "k5d4"):
        K, d = TAP_SETS[key]
        for P in (0, 1, (K - 1) * d - 1, (K - 1) * d):
            cases[f"p{P}_{key}"] = (2, 5, dr.window(K, d) + 6, K, d, P, P % 2 == 0, "")
    n = 0
    for key, (K, d) in TAP_SETS.items():
        w = dr.window(K, d)
        ts = [1, 2, w - 1, w, w + 1]
        if key == "k8d8":
            ts += [dr.FIR_TILE - 1, dr.FIR_TILE, dr.FIR_TILE + 1, 2 * dr.FIR_TILE + 3, dr.GRAD_TILE - 1, dr.GRAD_TILE, dr.GRAD_TILE + 1,
                   2 * dr.GRAD_TILE + 3]
        for T in sorted(set(t for t in ts if t >= 1)):
            cases[f"t{T}_{key}"] = (1 + n % 5, (8, 5, 12, 6, 3)[n % 5], T, K, d, (K - 1) * d, n % 2 == 0, "")
            n += 1
    for a in range(4):
        for b in range(4):
            cases[f"len{a}{b}"] = (2, 6, 40 + a, 5, 4, 16 - (a - b) % 4, (a + b) % 2 == 0, "")
    cases["fold9"] = (3, 6, 2 * dr.GRAD_TILE + 44, 8, 1, 7, True, "")
    cases["fold15"] = (5, 6, 2 * dr.GRAD_TILE + 3, 8, 1, 7, False, "")
    cases["fold20"] = (4, 3, 4 * dr.GRAD_TILE + 5, 3, 2, 4, True, "")
    cases["orth"] = (4, 16, 50, 8, 8, 56, True, "orth")
    cases["recipe_tcn"] = (256, 64, 100, 8, 8, 56, True, "")
    cases["recipe_mdtc"] = (100, 32, 200, 5, 8, 32, True, "")
    cases["long"] = (2, 5, 260, 32, 8, 248, True, "")
    return cases


CASES = _cases()


def case_names():
    return list(CASES)


@functools.lru_cache(maxsize=None)
def load_case(name):
    """-> dict(x (B, C, Tin), g (B, C, Tout), w (C, K), bias (C) or None, float32; d, P; backward: bool).  Read-only arrays."""
    B, C, Tin, K, d, P, has_bias, flavour = CASES[name]
    Tout = dr.tout(Tin, K, d, P)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = rng.standard_normal((B, C, Tin)).astype(np.float32)
    g = rng.standard_normal((B, C, Tout)).astype(np.float32)
    w = (0.3 * rng.standard_normal((C, K))).astype(np.float32)
    bias = (0.3 * rng.standard_normal(C)).astype(np.float32)
    if flavour == "nonfinite_x":
        x[0, :, 3] = np.nan
        x[1, :, 11] = np.inf
        x[1, ::2, 12] = -np.inf
    elif flavour == "inf_tap":
        w[1, 0] = np.inf                                           # tap 0 reads the padding for the first P frames
        w[2, 3] = -np.inf
    elif flavour == "orth":
        x[1::2] = x[0::2]
        g[1::2] = -(1.0 + 2.0 ** -12) * g[0::2]
    for a in (x, g, w, bias):
        a.setflags(write=False)
    return dict(x=x, g=g, w=w, bias=bias if has_bias else None, d=d, P=P, backward=name not in FORWARD_ONLY)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """-> (ref, mag): dicts over y, dx, dw, db (dx, dw, db only where the case runs backward), float64.  db does not depend on
    there being a bias: the C entry point gives it either way, torch only with one."""
    c = load_case(name)
    y, ym = dr.forward(c["x"], c["w"], c["bias"], c["d"], c["P"])
    ref, mag = {"y": y}, {"y": ym}
    if c["backward"]:
        r, m = dr.backward(c["x"], c["g"], c["w"], c["d"], c["P"])
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
    """got: dict over a subset of y, dx, dw, db -> (dict of worst units, list of quantities whose classes differ)."""
    ref, mag = oracle(name)
    out, bad = {}, []
    for k, v in got.items():
        v = np.asarray(v).reshape(ref[k].shape)
        if not same_classes(v, ref[k]):
            bad.append(k)
        out[k] = worst_units(v, ref[k], mag[k])
    return out, bad


def device_dw_bound(name):
    """The device's own bound on dw and db in the units above.  The products of two floats are exact in double and the sums are
    double, so what the device loses is N roundings of 2^-53 relative to sum|terms| (N = B Tout terms a tap) and one final
    rounding to float32: at most 2^-24 of the result, so at most one unit.  The oracle's own float64 sum is allowed as much
    again."""
    B, _, Tin, K, d, P = CASES[name][:6]
    return 1.0 + 2.0 * B * dr.tout(Tin, K, d, P) * 2.0 ** -53 / U
