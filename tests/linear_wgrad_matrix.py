"""Case list, units, bars and the element bound of the Linear weight-gradient tests (tests/test_linear_wgrad_ref.py on the CPU,
tests/test_hip_linear_wgrad.py on the GPU).  The oracle and the emulation of the kernel's arithmetic are tests/linear_wgrad_ref.py.

Shapes are (R, O, I): x (R, I), g (R, O), dw (O, I) = g^T x, db (O) = sum_r g.  Seeded, x and g ~ N(0, 1).  K is the plan's chain
length, read through wekws_hip_linear_wgrad_plan, so the cases follow it (K = 512 today); a stage is 32 rows, an MFMA tile 16 x 16,
a workgroup's tile 64 x 64.

    r1 r31 r32 r33 rK-1 rK rK+1 r2K+1     at (., 16, 16): less than a stage, a stage and its edges, a chain and its edges, three
                                          chains in three slices with a ragged last one of a single row
    slices           (16 K + 5, 2, 2049): 33 tiles, so slices of two chains each and a last slice of one ragged chain
    o<O>i<I>         O, I in 1, 15, 16, 17, 63, 64, 65 crossed sparsely at R = 70: the MFMA tile's and the workgroup tile's edges,
                     the scalar fetch (O or I no multiple of 4) and the 16-byte fetch
    odd              (1000, 130, 67): several tiles each way, ragged both ways, two chains, scalar fetch
    nobias           db not wanted;          now: dw not wanted (only the bias column's workgroups run)
    unaligned        x and g at a base 4 bytes past a 16-byte boundary with O and I multiples of 4: the scalar fetch by alignment
    nan              a NaN at x[NAN_R][NAN_I]: column NAN_I of dw is NaN, every other column and db have the clean run's bits
    inf              +Inf at g[INF_R][INF_O]: the classes of row INF_O of dw and of db[INF_O] are the oracle's
    large            x and g scaled by 2^40: products near 2^80, no overflow
    gru_ih fsmn_in fsmn_blk cls           the recipes' shapes: (25600, 384, 128), (25600, 140, 400), (25600, 128, 250),
                                          (4096, 2599, 140)

Units, per tensor, U = 2^-24: max|got - ref64| / (U max|ref64|) over the finite elements (gru_train_matrix.tensor_units); the
classes (NaN, +Inf, -Inf) are compared first and exactly.

BARS -- the project's rule: pow2_at_or_above(4 x the worst units of torch's CPU float32 ``g.t().mm(x)`` and ``g.sum(0)`` over
this matrix, one thread); tests/test_linear_wgrad_ref.py recomputes the table:

    quantity   torch's worst units (case)   bar
    dw         8.62  (gru_ih)               64
    db         4.14  (r2K+1)                32

(The emulation of the kernel's arithmetic, tests/linear_wgrad_ref.py, is at most 13.8 units for dw and 10.9 for db on the cases
it is run on: the bars can be met by 512-row chains.)

The element bound: every element is also held to the bound of the kernel's own arithmetic,

    |got - ref| <= U |ref| + gamma(K) sum_r |g[r][o] x[r][i]|,       gamma(n) = (n + 1) U / (1 - (n + 1) U).

Derivation.  A chain is n <= K float32 fmaf steps; step k computes (acc + g x)(1 + d_k), |d_k| <= U, so a product meets at most
n factors (1 + d) and the chain's error is at most gamma_n sum |g x| over its rows, gamma_n = n U / (1 - n U) (Higham, Accuracy
and Stability of Numerical Algorithms, Lemma 3.1 and section 3.1).  Chains cover disjoint rows, so over all chains the error is at
most gamma_K sum_r |g x|.  The doubles that add the chains and the slices round (chains + slices) times at 2^-53 each, far below
one further U on the same sum as long as chains + slices < 2^28; the last rounding to float32 costs U |S| with
|S| <= |ref| + the error so far, and that cross term is below U^2 (K + 1) sum |g x|.  One more U in gamma -- n + 1 for n -- covers
both.  The bias is the same chain with x = 1.  The bound is about (1 + K) U relative to sum |g x|: what a kernel with float16 or
bfloat16 products, or with one float32 chain over all R rows, does not meet.

The negative control: x rounded to float16, through the oracle itself, at gru_ih must miss the dw bar by a factor of 8 at least
(CONTROL_UNITS).
"""
from __future__ import annotations

import ctypes
import functools
import zlib

import numpy as np

from tests import linear_wgrad_ref as lr
from tests.gru_train_matrix import same_classes, tensor_units  # noqa: F401 (the units are the GRU tests')

U = 2.0 ** -24
QUANTITIES = ("dw", "db")
# measured by tests/test_linear_wgrad_ref.py::test_bars_are_recomputed (its -s output)
REF_UNITS = {"dw": 8.62, "db": 4.14}
BARS = {"dw": 64.0, "db": 32.0}              # pow2_at_or_above(4 x REF_UNITS)
CONTROL_UNITS = 3901.1                       # dw at gru_ih with x rounded to float16, against the oracle
NAN_R, NAN_I = 37, 5
INF_R, INF_O = 11, 3
RECIPE = {"gru_ih": (25600, 384, 128), "fsmn_in": (25600, 140, 400), "fsmn_blk": (25600, 128, 250), "cls": (4096, 2599, 140)}


@functools.lru_cache(maxsize=None)
def device_plan(R, O, I):
    """wekws_hip_linear_wgrad_plan, without a device -> dict(chain, chains, slices, chains_per_slice, grid, workspace_bytes)."""
    from wekws_amd import _capi
    out = (ctypes.c_int64 * 5)()
    rc = _capi.load().wekws_hip_linear_wgrad_plan(R, O, I, out)
    assert rc == 0, _capi.last_error()
    p = lr.plan_of(out[0], out[1], out[2])
    p.update(grid=int(out[3]), workspace_bytes=int(out[4]))
    return p


def chain_rows():
    return device_plan(1, 1, 1)["chain"]


def _c(R, O, I, flavour="", bias=True, weight=True):
    return dict(R=R, O=O, I=I, flavour=flavour, bias=bias, weight=weight)


@functools.lru_cache(maxsize=None)
def cases():
    K = chain_rows()
    out = {}
    for name, R in (("r1", 1), ("r31", 31), ("r32", 32), ("r33", 33), ("rK-1", K - 1), ("rK", K), ("rK+1", K + 1), ("r2K+1", 2 * K + 1)):
        out[name] = _c(R, 16, 16)
    out["slices"] = _c(16 * K + 5, 2, 2049)
    for O, I in ((1, 65), (15, 16), (16, 17), (17, 15), (63, 64), (64, 63), (64, 64), (65, 1), (65, 65)):
        out[f"o{O}i{I}"] = _c(70, O, I)
    out["odd"] = _c(1000, 130, 67)
    out["nobias"] = _c(100, 20, 24, bias=False)
    out["now"] = _c(100, 20, 24, weight=False)
    out["unaligned"] = _c(100, 16, 16, flavour="unaligned")
    out["nan"] = _c(100, 20, 24, flavour="nan")
    out["inf"] = _c(100, 20, 24, flavour="inf")
    out["large"] = _c(600, 20, 24, flavour="large")
    for name, (R, O, I) in RECIPE.items():
        out[name] = _c(R, O, I, flavour="recipe")
    return out


def case_names():
    return list(cases())


def small_case_names():
    return [n for n, s in cases().items() if s["flavour"] != "recipe"]


@functools.lru_cache(maxsize=None)
def load_case(name):
    """-> dict(spec, x (R, I), g (R, O)) float32, read-only."""
    s = cases()[name]
    rng = np.random.default_rng(zlib.crc32(("linear_wgrad/" + name).encode()))
    x = rng.standard_normal((s["R"], s["I"])).astype(np.float32)
    g = rng.standard_normal((s["R"], s["O"])).astype(np.float32)
    if s["flavour"] == "nan":
        x[NAN_R, NAN_I] = np.nan
    elif s["flavour"] == "inf":
        g[INF_R, INF_O] = np.inf
    elif s["flavour"] == "large":
        x *= np.float32(2.0 ** 40)
        g *= np.float32(2.0 ** 40)
    x.setflags(write=False)
    g.setflags(write=False)
    return dict(spec=s, x=x, g=g)


def quantities(name):
    s = cases()[name]
    return [q for q in QUANTITIES if (q == "dw" and s["weight"]) or (q == "db" and s["bias"])]


@functools.lru_cache(maxsize=None)
def oracle(name):
    c = load_case(name)
    out = lr.oracle(c["x"], c["g"])
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def emulated(name):
    c, s = load_case(name), cases()[name]
    dw, db = lr.emulate(c["x"], c["g"], device_plan(s["R"], s["O"], s["I"]))
    dw.setflags(write=False)
    db.setflags(write=False)
    return dict(dw=dw, db=db)


def gamma(n):
    return (n + 1) * U / (1.0 - (n + 1) * U)


def units(name, got):
    """got: dict over a subset of the quantities -> (dict of units, list of quantities whose classes differ)."""
    ref = oracle(name)
    out, bad = {}, []
    for q, a in got.items():
        a = np.asarray(a).reshape(ref[q].shape)
        if not same_classes(a, ref[q]):
            bad.append(q)
        out[q] = tensor_units(a, ref[q])
    return out, bad


def element_excess(name, got):
    """got: dict over a subset of the quantities -> dict of max over the finite elements of |got - ref| / bound (<= 1 passes;
    0 where nothing is finite)."""
    ref = oracle(name)
    g_k = gamma(chain_rows())
    out = {}
    for q, a in got.items():
        r, mag = ref[q], ref["abs_" + q]
        a = np.asarray(a, np.float64).reshape(r.shape)
        fin = np.isfinite(r) & np.isfinite(a) & np.isfinite(mag)
        if not fin.any():
            out[q] = 0.0
            continue
        err, bound = np.abs(a[fin] - r[fin]), U * np.abs(r[fin]) + g_k * mag[fin]
        zero = bound == 0
        worst = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
        if (err[zero] != 0).any():
            worst = float("inf")
        out[q] = worst
    return out
