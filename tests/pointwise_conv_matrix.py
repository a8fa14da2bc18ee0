"""Case list, units, bars and the element bounds of the pointwise Conv1d tests (tests/test_pointwise_conv_ref.py on the CPU,
tests/test_hip_pointwise_conv.py on the GPU).  The oracle and the emulation of the kernels' arithmetic are
tests/pointwise_conv_ref.py.

Shapes are (B, Ci, Co, T): x (B, Ci, T), g (B, Co, T), w (Co, Ci), bias (Co); y = w x + bias, dx = w^T g, dw = sum_{b,t} g x,
db = sum_{b,t} g.  Seeded, everything ~ N(0, 1).  K is the plan's chain length, read through wekws_hip_pointwise_conv1d_plan, so
the cases follow it (K = 512 today); a stage is 32 channels (forward, dx) or 32 rows r = b T + t (dw, db), an MFMA tile 16 x 16, a
workgroup's tile 64 x 64.

    t1 t15 t16 t17 t63 t64 t65 t129       at (2, 16, 16, .): the MFMA tile's and the workgroup tile's frame edges, the scalar
                                          fetch (T no multiple of 4) and the 16-byte fetch
    i<Ci>o<Co>       Ci, Co in 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65 crossed sparsely at B = 2, T = 35: the channel edges
                     of the MFMA's k, of the stage and of both tiles; the weight's scalar and 16-byte fetch
    ragged           (3, 130, 67, 70): several tiles each way, ragged every way
    chain600         (3, 8, 8, 200): R = 600, the chain boundary at K = 512 falls inside batch row 2
    straddle         (5, 4, 4, 103): stages straddle batch rows, T % 4 != 0
    rK-1 rK rK+1 r2K+1   (B, 8, 8, T) with B T = K - 1, K, K + 1, 2 K + 1 (B the smallest divisor above 1)
    slices           (7, 2049, 2, (16 K + 5) / 7): 33 tiles of dw, so slices of two chains each and a last slice of one ragged chain
    nobias           no bias;      nodx nodw nodb: that gradient not wanted
    unaligned        x, g, w at bases 4 bytes past a 16-byte boundary with T and Ci multiples of 4: the scalar fetch by alignment
    nan              a NaN at x[NAN_B][NAN_I][NAN_T]: y[NAN_B][:, NAN_T] and column NAN_I of dw are NaN, everything else has the
                     clean run's bits
    inf              +Inf at g[INF_B][INF_O][INF_T]: the classes of dx, dw and db are the oracle's
    large            x, w and g scaled by 2^40: products near 2^80, no overflow
    ds_tcn mdtc mdtc_pre ds256            the recipes' shapes: (256, 64, 64, 100), (100, 32, 32, 200), (100, 80, 32, 200),
                                          (256, 256, 256, 100)

Units, per tensor, U = 2^-24: max|got - ref64| / (U max|ref64|) over the finite elements (gru_train_matrix.tensor_units); the
classes (NaN, +Inf, -Inf) are compared first and exactly.

BARS -- the project's rule, per quantity: pow2_at_or_above(4 x the worst units of torch's CPU float32 ``F.conv1d`` and its
autograd over this matrix, one thread); tests/test_pointwise_conv_ref.py recomputes the table:

    quantity   torch's worst units (case)   bar
    y          11.85 (ds256)                64
    dx         13.22 (ds256)                64
    dw         10.62 (ds_tcn)               64
    db         62.51 (ds_tcn)               256

The element bounds: every element is also held to the bound of the kernels' own arithmetic, with the standard
gamma_n = n U / (1 - n U) (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1):

    y     |got - ref| <= U |ref| + gamma_{Ci+1} (sum_i |w[o][i] x[b][i][t]| + |bias[o]|)
    dx    |got - ref| <= U |ref| + gamma_{Co+1} sum_o |w[o][i] g[b][o][t]|
    dw    |got - ref| <= U |ref| + gamma(K) sum_r |g x|     (tests/linear_wgrad_matrix.py's bound and its gamma, unchanged)
    db    |got - ref| <= U |ref| + gamma(K) sum_r |g|

Derivation for y.  The chain is n = Ci float32 fmaf steps from +0; step k computes (acc + w x)(1 + d_k), |d_k| <= U, so a
product meets at most n factors (1 + d) and the chain's value is sum_i w x (1 + theta_i) with |theta_i| <= gamma_n.  The bias
addition is one more rounding: got = (chain + bias)(1 + d).  Hence got - ref = d ref + (1 + d) sum_i w x theta_i and
|got - ref| <= U |ref| + (1 + U) gamma_n sum |w x| <= U |ref| + gamma_{n+1} sum |w x| (Higham, Lemma 3.3: (1 + U) gamma_n <=
gamma_{n+1}).  Adding |bias| to the sum only loosens the bound by gamma_{n+1} |bias| and keeps the form the same with and without
a bias.  dx is the same chain over o without the last addition.  The bound is about Ci U relative to sum |w x|: what a kernel
with float16 or bfloat16 products does not meet.

The negative control: w rounded to float16, through the oracle itself, at ds_tcn must miss the y bar by a factor of 8 at least
(CONTROL_UNITS).
"""
from __future__ import annotations

import ctypes
import functools
import zlib

import numpy as np

from tests import linear_wgrad_matrix as lm
from tests import linear_wgrad_ref as lr
from tests import pointwise_conv_ref as pr
from tests.gru_train_matrix import same_classes, tensor_units  # noqa: F401 (the units are the GRU tests')

U = 2.0 ** -24
QUANTITIES = ("y", "dx", "dw", "db")
# measured by tests/test_pointwise_conv_ref.py::test_bars_are_recomputed (its -s output)
REF_UNITS = {"y": 11.85, "dx": 13.22, "dw": 10.62, "db": 62.51}
BARS = {"y": 64.0, "dx": 64.0, "dw": 64.0, "db": 256.0}       # pow2_at_or_above(4 x REF_UNITS)
CONTROL_UNITS = 3509.0                       # y at ds_tcn with w rounded to float16, against the oracle
CONTROL_CASE = "ds_tcn"
NAN_B, NAN_I, NAN_T = 1, 5, 37
INF_B, INF_O, INF_T = 1, 3, 11
RECIPE = {"ds_tcn": (256, 64, 64, 100), "mdtc": (100, 32, 32, 200), "mdtc_pre": (100, 80, 32, 200), "ds256": (256, 256, 256, 100)}
CHANNEL_PAIRS = ((1, 65), (3, 4), (4, 5), (5, 3), (15, 16), (16, 17), (17, 15), (31, 32), (32, 33), (33, 31), (63, 64), (64, 63),
                 (64, 64), (65, 1), (65, 65))
# the cases recorded from the live reference in tests/golden/pointwise_conv_golden.npz -> the module that ran them
GOLDEN = {"t17": "ds", "i16o17": "dsd", "i5o3": "dsd", "nobias": "dsd_nobias", "straddle": "tcnblock", "chain600": "ds"}


@functools.lru_cache(maxsize=None)
def device_plan(B, Ci, T, Co):
    """wekws_hip_pointwise_conv1d_plan, without a device -> dict(chain, chains, slices, chains_per_slice, grid,
    workspace_bytes, forward_grid, dx_grid)."""
    from wekws_amd import _capi
    out = (ctypes.c_int64 * 7)()
    rc = _capi.load().wekws_hip_pointwise_conv1d_plan(B, Ci, T, Co, out)
    assert rc == 0, _capi.last_error()
    p = lr.plan_of(out[0], out[1], out[2])
    p.update(grid=int(out[3]), workspace_bytes=int(out[4]), forward_grid=int(out[5]), dx_grid=int(out[6]))
    return p


def chain_rows():
    return device_plan(1, 1, 1, 1)["chain"]


def _c(B, Ci, Co, T, flavour="", bias=True, wants=("dx", "dw", "db")):
    return dict(B=B, Ci=Ci, Co=Co, T=T, flavour=flavour, bias=bias, wants=tuple(q for q in wants if bias or q != "db"))


def _split(R):
    """R = B T with B the smallest divisor of R above 1 (1 if R is prime)."""
    B = next((d for d in range(2, int(R ** 0.5) + 1) if R % d == 0), 1)
    return B, R // B


@functools.lru_cache(maxsize=None)
def cases():
    K = chain_rows()
    out = {}
    for T in (1, 15, 16, 17, 63, 64, 65, 129):
        out[f"t{T}"] = _c(2, 16, 16, T)
    for Ci, Co in CHANNEL_PAIRS:
        out[f"i{Ci}o{Co}"] = _c(2, Ci, Co, 35)
    out["ragged"] = _c(3, 130, 67, 70)
    out["chain600"] = _c(3, 8, 8, 200)
    out["straddle"] = _c(5, 4, 4, 103)
    for name, R in (("rK-1", K - 1), ("rK", K), ("rK+1", K + 1), ("r2K+1", 2 * K + 1)):
        B, T = _split(R)
        out[name] = _c(B, 8, 8, T)
    B, T = _split(16 * K + 5)
    out["slices"] = _c(B, 2049, 2, T)
    out["nobias"] = _c(2, 20, 24, 50, bias=False)
    out["nodx"] = _c(2, 20, 24, 50, wants=("dw", "db"))
    out["nodw"] = _c(2, 20, 24, 50, wants=("dx", "db"))
    out["nodb"] = _c(2, 20, 24, 50, wants=("dx", "dw"))
    out["unaligned"] = _c(2, 16, 16, 36, flavour="unaligned")
    out["nan"] = _c(2, 20, 24, 50, flavour="nan")
    out["inf"] = _c(2, 20, 24, 50, flavour="inf")
    out["large"] = _c(3, 20, 24, 200, flavour="large")
    for name, (B, Ci, Co, T) in RECIPE.items():
        out[name] = _c(B, Ci, Co, T, flavour="recipe")
    return out


def case_names():
    return list(cases())


def small_case_names():
    return [n for n, s in cases().items() if s["flavour"] != "recipe"]


@functools.lru_cache(maxsize=None)
def load_case(name):
    """-> dict(spec, x (B, Ci, T), g (B, Co, T), w (Co, Ci), bias (Co) or None) float32, read-only."""
    s = cases()[name]
    rng = np.random.default_rng(zlib.crc32(("pointwise_conv/" + name).encode()))
    x = rng.standard_normal((s["B"], s["Ci"], s["T"])).astype(np.float32)
    g = rng.standard_normal((s["B"], s["Co"], s["T"])).astype(np.float32)
    w = rng.standard_normal((s["Co"], s["Ci"])).astype(np.float32)
    bias = rng.standard_normal(s["Co"]).astype(np.float32) if s["bias"] else None
    if s["flavour"] == "nan":
        x[NAN_B, NAN_I, NAN_T] = np.nan
    elif s["flavour"] == "inf":
        g[INF_B, INF_O, INF_T] = np.inf
    elif s["flavour"] == "large":
        for a in (x, g, w):
            a *= np.float32(2.0 ** 40)
    for a in (x, g, w, bias):
        if a is not None:
            a.setflags(write=False)
    return dict(spec=s, x=x, g=g, w=w, bias=bias)


def quantities(name):
    return ["y"] + [q for q in QUANTITIES[1:] if q in cases()[name]["wants"]]


@functools.lru_cache(maxsize=None)
def oracle(name):
    c = load_case(name)
    out = pr.oracle(c["x"], c["w"], c["bias"], c["g"])
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def emulated(name):
    """All four quantities (db without a bias too: the column sums of g)."""
    c, s = load_case(name), cases()[name]
    dw, db = pr.emulate_wgrad(c["x"], c["g"], device_plan(s["B"], s["Ci"], s["T"], s["Co"]))
    out = dict(y=pr.emulate_forward(c["x"], c["w"], c["bias"]), dx=pr.emulate_dx(c["g"], c["w"]), dw=dw, db=db)
    for a in out.values():
        a.setflags(write=False)
    return out


def gamma_std(n):
    return n * U / (1.0 - n * U)


def _gamma(name, q):
    s = cases()[name]
    return {"y": gamma_std(s["Ci"] + 1), "dx": gamma_std(s["Co"] + 1)}.get(q, lm.gamma(chain_rows()))


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
    out = {}
    for q, a in got.items():
        r, mag = ref[q], ref["abs_" + q]
        a = np.asarray(a, np.float64).reshape(r.shape)
        fin = np.isfinite(r) & np.isfinite(a) & np.isfinite(mag)
        if not fin.any():
            out[q] = 0.0
            continue
        err, bound = np.abs(a[fin] - r[fin]), U * np.abs(r[fin]) + _gamma(name, q) * mag[fin]
        zero = bound == 0
        worst = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
        if (err[zero] != 0).any():
            worst = float("inf")
        out[q] = worst
    return out
