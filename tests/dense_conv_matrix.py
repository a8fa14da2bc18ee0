"""Case list, units, bars and the element bounds of the dense Conv1d tests (tests/test_dense_conv_ref.py on the CPU,
tests/test_hip_dense_conv.py on the GPU).  The oracle and the emulation of the kernels' arithmetic are tests/dense_conv_ref.py.

A case is (B, Ci, Co, Tin, K, d, P): x (B, Ci, Tin), w (Co, Ci, K), bias (Co), g (B, Co, Tout), Tout = Tin + P - (K - 1) d;
y = conv(pad(x, (P, 0)), w, bias, dilation=d) and its gradients for the upstream gradient g.  Seeded by name, everything
~ N(0, 1).  The chain length is the plan's, read through wekws_hip_dense_conv1d_plan, so the cases follow it (512 today); a stage
is 32 channels of one tap (forward, dx) or 32 rows r = b Tout + t (dw, db), an MFMA tile 16 x 16, a workgroup's tile 64 x 64.
"full" is P = (K - 1) d, the CnnBlock's padding.

    t1 t15 t16 t17 t63 t64 t65 t129   Tout at (2, 16, 16), K = 3, d = 2, full: the MFMA tile's and the workgroup tile's frame edges;
                                      shifts -4, -2, 0: the 16-byte fetch and the scalar one (Tin = Tout a multiple of 4 or not)
    k1                 K = 1 (the pointwise product): (2, 20, 24, 50)
    k2d3 k3d3 k3d3p2 k3d8 k8d1 k8d1p3 k8d1p0 k8d2 k8d8
                       K in 2, 3, 8 and d in 1, 2, 3, 8 with P zero, partial and full; k8d1p3 has the shifts k - 3 = -3 .. 4: every
                       residue mod 4 with both signs
    subsampling        the Conv1dSubsampling1 shape: (2, 20, 24, 50), K = 3, d = 1, P = 0, Ci != Co
    short              Tin = 3 shorter than the padding: K = 8, d = 1, P = 7
    window_k2 window_k32   the largest window, 256 frames: K = 2, d = 255 and K = 32, d = 8, full, at 3 -> 2 and 2 -> 3 channels
    i<Ci>o<Co>         Ci, Co in 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65 crossed sparsely (pointwise_conv_matrix's
                       CHANNEL_PAIRS) at B = 2, Tin = 35, K = 3, d = 2, full
    chain600           (3, 8, 8, 200), K = 3, d = 2, full: R = 600, the chain boundary at 512 falls inside batch row 2
    straddle           (5, 4, 4, 103), K = 3, d = 1, full: stages straddle batch rows, Tout % 4 != 0
    rK-1 rK rK+1 r2K+1 (B, 8, 8, T), K = 2, d = 1, full, with B Tout = chain - 1, chain, chain + 1, 2 chain + 1
    slices             (5, 1025, 2, (30 chain + 5) / 5), K = 2, d = 1, full: 17 tiles of dw[:, :, k] and 31 chains, so slices of two
                       chains each and a last slice of one ragged chain; K Ci = 2050, the longest chain of the pointwise matrix (2049)
    nobias             no bias;      nodx nodw nodb: that gradient not wanted
    unaligned          x, g, w at bases 4 bytes past a 16-byte boundary with Tin a multiple of 4: the scalar fetch by alignment
    nan                a NaN at x[NAN_B][NAN_I][Tin - 2] with K = 3, d = 2, full: the y columns whose window holds it and dw[:, NAN_I, k]
                       of the taps that reach it (the last one alone) are NaN, everything else has the clean run's bits
    inf                +Inf at g[INF_B][INF_O][INF_T]: the classes of dx, dw and db are the oracle's
    winf               +Inf at w[WINF_O][WINF_I][0] with P = 4, forward only: NaN over the padding (t < 4), as the reference
    large              x, w and g scaled by 2^40: products near 2^80, no overflow
    tcn_d1 tcn_d2 tcn_d4 tcn_d8   the recipe's four layers: (256, 64, 64, 100), K = 8, full

Units, per tensor, U = 2^-24: max|got - ref64| / (U max|ref64|) over the finite elements (gru_train_matrix.tensor_units); the
classes (NaN, +Inf, -Inf) are compared first and exactly.

BARS -- the project's rule, per quantity: pow2_at_or_above(4 x the worst units of torch's CPU float32 ``F.conv1d`` and its
autograd over this matrix, one thread); tests/test_dense_conv_ref.py recomputes the table:

    quantity   torch's worst units (case)   bar
    y          6.93 (k8d1p0)                32
    dx         6.87 (k8d1)                  32
    dw         124.29 (tcn_d4)              512
    db         83.93 (tcn_d4)               512

The element bounds: every element is also held to the bound of the kernels' own arithmetic, with the standard
gamma_n = n U / (1 - n U) (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1):

    y     |got - ref| <= U |ref| + gamma_{K Ci + 1} (sum_{k,i} |w[o][i][k] xp[b][i][t + k d - P]| + |bias[o]|)
    dx    |got - ref| <= U |ref| + gamma_{K Co + 1} sum_{k,o} |w[o][i][k] g[b][o][n + P - k d]|
    dw    |got - ref| <= U |ref| + gamma(chain) sum_r |g xp|     (tests/linear_wgrad_matrix.py's bound and its gamma, unchanged)
    db    |got - ref| <= U |ref| + gamma(chain) sum_r |g|

The derivation is tests/pointwise_conv_matrix.py's with a chain of n = K Ci (K Co) fmaf steps instead of Ci (Co): the padding's
zeros are exact products and add nothing to either side.

The negative control: w rounded to float16, through the oracle itself, at tcn_d4 must miss the y bar by a factor of 8 at least
(CONTROL_UNITS).
"""
from __future__ import annotations

import ctypes
import functools
import zlib

import numpy as np

from tests import dense_conv_ref as dr
from tests import linear_wgrad_matrix as lm
from tests import linear_wgrad_ref as lr
from tests.gru_train_matrix import same_classes, tensor_units  # noqa: F401 (the units are the GRU tests')
from tests.pointwise_conv_matrix import CHANNEL_PAIRS

U = 2.0 ** -24
QUANTITIES = ("y", "dx", "dw", "db")
# measured by tests/test_dense_conv_ref.py::test_bars_are_recomputed (its -s output)
REF_UNITS = {"y": 6.93, "dx": 6.87, "dw": 124.29, "db": 83.93}
BARS = {"y": 32.0, "dx": 32.0, "dw": 512.0, "db": 512.0}       # pow2_at_or_above(4 x REF_UNITS)
CONTROL_UNITS = 3622.0                          # y at tcn_d4 with w rounded to float16, against the oracle
CONTROL_CASE = "tcn_d4"
NAN_B, NAN_I = 1, 5
INF_B, INF_O, INF_T = 1, 3, 11
WINF_O, WINF_I = 2, 7
RECIPE = {f"tcn_d{d}": (256, 64, 64, 100, 8, d, 7 * d) for d in (1, 2, 4, 8)}
# the cases recorded from the live reference in tests/golden/dense_conv_golden.npz -> the module that ran them
GOLDEN = {"t17": "cnn", "k8d2": "cnn", "k8d8": "cnn", "straddle": "cnn", "subsampling": "subsampling1"}


@functools.lru_cache(maxsize=None)
def device_plan(B, Ci, Tin, Co, K, d, P):
    """wekws_hip_dense_conv1d_plan, without a device -> dict(chain, chains, slices, chains_per_slice, grid, workspace_bytes,
    forward_grid, dx_grid, taps, fold_grid, Tout)."""
    from wekws_amd import _capi
    out = (ctypes.c_int64 * 10)()
    rc = _capi.load().wekws_hip_dense_conv1d_plan(B, Ci, Tin, Co, K, d, P, out)
    assert rc == 0, _capi.last_error()
    p = lr.plan_of(out[0], out[1], out[2])
    p.update(grid=int(out[3]), workspace_bytes=int(out[4]), forward_grid=int(out[5]), dx_grid=int(out[6]), taps=int(out[7]),
             fold_grid=int(out[8]), Tout=int(out[9]))
    return p


def chain_rows():
    return device_plan(1, 1, 1, 1, 1, 1, 0)["chain"]


def _c(B, Ci, Co, Tin, K, d, P=None, flavour="", bias=True, wants=("dx", "dw", "db")):
    P = (K - 1) * d if P is None else P
    return dict(B=B, Ci=Ci, Co=Co, Tin=Tin, K=K, d=d, P=P, Tout=dr.tout(Tin, K, d, P), flavour=flavour, bias=bias,
                wants=tuple(q for q in wants if bias or q != "db"))


def _split(R):
    """R = B T with B the smallest divisor of R above 1 (1 if R is prime)."""
    B = next((d for d in range(2, int(R ** 0.5) + 1) if R % d == 0), 1)
    return B, R // B


@functools.lru_cache(maxsize=None)
def cases():
    chain = chain_rows()
    out = {}
    for T in (1, 15, 16, 17, 63, 64, 65, 129):
        out[f"t{T}"] = _c(2, 16, 16, T, 3, 2)
    out["k1"] = _c(2, 20, 24, 50, 1, 1)
    out["k2d3"] = _c(2, 16, 16, 40, 2, 3)
    out["k3d3"] = _c(2, 16, 16, 40, 3, 3, P=0)
    out["k3d3p2"] = _c(2, 16, 16, 40, 3, 3, P=2)
    out["k3d8"] = _c(2, 16, 16, 40, 3, 8)
    out["k8d1"] = _c(2, 16, 16, 40, 8, 1)
    out["k8d1p3"] = _c(2, 16, 16, 40, 8, 1, P=3)
    out["k8d1p0"] = _c(2, 16, 16, 40, 8, 1, P=0)
    out["k8d2"] = _c(2, 16, 16, 40, 8, 2)
    out["k8d8"] = _c(2, 8, 8, 100, 8, 8)
    out["subsampling"] = _c(2, 20, 24, 50, 3, 1, P=0)
    out["short"] = _c(2, 16, 16, 3, 8, 1)
    out["window_k2"] = _c(2, 3, 2, 40, 2, 255)
    out["window_k32"] = _c(2, 2, 3, 20, 32, 8)
    for Ci, Co in CHANNEL_PAIRS:
        out[f"i{Ci}o{Co}"] = _c(2, Ci, Co, 35, 3, 2)
    out["chain600"] = _c(3, 8, 8, 200, 3, 2)
    out["straddle"] = _c(5, 4, 4, 103, 3, 1)
    for name, R in (("rK-1", chain - 1), ("rK", chain), ("rK+1", chain + 1), ("r2K+1", 2 * chain + 1)):
        B, T = _split(R)
        out[name] = _c(B, 8, 8, T, 2, 1)
    B, T = _split(30 * chain + 5)
    out["slices"] = _c(B, 1025, 2, T, 2, 1)
    out["nobias"] = _c(2, 20, 24, 50, 3, 2, bias=False)
    out["nodx"] = _c(2, 20, 24, 50, 3, 2, wants=("dw", "db"))
    out["nodw"] = _c(2, 20, 24, 50, 3, 2, wants=("dx", "db"))
    out["nodb"] = _c(2, 20, 24, 50, 3, 2, wants=("dx", "dw"))
    out["unaligned"] = _c(2, 16, 16, 36, 3, 2, flavour="unaligned")
    out["nan"] = _c(2, 20, 24, 50, 3, 2, flavour="nan")
    out["inf"] = _c(2, 20, 24, 50, 3, 2, flavour="inf")
    out["winf"] = _c(2, 20, 24, 50, 3, 2, flavour="winf", wants=())
    out["large"] = _c(3, 20, 24, 200, 3, 2, flavour="large")
    for name, (B, Ci, Co, Tin, K, d, P) in RECIPE.items():
        out[name] = _c(B, Ci, Co, Tin, K, d, P, flavour="recipe")
    return out


def case_names():
    return list(cases())


def small_case_names():
    return [n for n, s in cases().items() if s["flavour"] != "recipe"]


def nan_frame(s):
    return s["Tin"] - 2


def nan_hits(s):
    """-> (the y frames whose window holds the NaN's frame, the taps that reach it)."""
    n = nan_frame(s)
    frames = [n + s["P"] - k * s["d"] for k in range(s["K"])]
    taps = [k for k, t in enumerate(frames) if 0 <= t < s["Tout"]]
    return [frames[k] for k in taps], taps


@functools.lru_cache(maxsize=None)
def load_case(name):
    """-> dict(spec, x (B, Ci, Tin), g (B, Co, Tout), w (Co, Ci, K), bias (Co) or None) float32, read-only."""
    s = cases()[name]
    rng = np.random.default_rng(zlib.crc32(("dense_conv/" + name).encode()))
    x = rng.standard_normal((s["B"], s["Ci"], s["Tin"])).astype(np.float32)
    g = rng.standard_normal((s["B"], s["Co"], s["Tout"])).astype(np.float32)
    w = rng.standard_normal((s["Co"], s["Ci"], s["K"])).astype(np.float32)
    bias = rng.standard_normal(s["Co"]).astype(np.float32) if s["bias"] else None
    if s["flavour"] == "nan":
        x[NAN_B, NAN_I, nan_frame(s)] = np.nan
    elif s["flavour"] == "inf":
        g[INF_B, INF_O, INF_T] = np.inf
    elif s["flavour"] == "winf":
        w[WINF_O, WINF_I, 0] = np.inf
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
    c, s = load_case(name), cases()[name]
    out = dr.oracle(c["x"], c["w"], c["bias"], c["g"], s["d"], s["P"])
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def emulated(name):
    """The quantities of the case and db without a bias too (the column sums of g); a forward-only case has y alone."""
    c, s = load_case(name), cases()[name]
    out = dict(y=dr.emulate_forward(c["x"], c["w"], c["bias"], s["d"], s["P"]))
    if s["wants"]:
        dw, db = dr.emulate_wgrad(c["x"], c["g"], s["d"], s["P"], s["K"],
                                  device_plan(s["B"], s["Ci"], s["Tin"], s["Co"], s["K"], s["d"], s["P"]))
        out.update(dx=dr.emulate_dx(c["g"], c["w"], s["d"], s["P"], s["Tin"]), dw=dw, db=db)
    for a in out.values():
        a.setflags(write=False)
    return out


def gamma_std(n):
    return n * U / (1.0 - n * U)


def _gamma(name, q):
    s = cases()[name]
    return {"y": gamma_std(s["K"] * s["Ci"] + 1), "dx": gamma_std(s["K"] * s["Co"] + 1)}.get(q, lm.gamma(chain_rows()))


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
