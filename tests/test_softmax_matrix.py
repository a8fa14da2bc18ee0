"""CPU: the softmax matrix (tests/softmax_matrix.py) is what it says it is; the calibration of K_SOFTMAX (tests/helpers.py) from two
plain float32 evaluations; the negative controls of the bar, as emulations of the kernels' order of operations; the float64
oracle's top-k against the float32 one that the goldens pin."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import topk_oracle
from tests import softmax_matrix as sm
from tests.fbank_matrix import hooks_path
from tests.helpers import CONTROL_MARGIN, K_SOFTMAX, pow2_at_or_above
from wekws_amd import _capi


def aten_f32(x):
    return torch.softmax(torch.from_numpy(x), -1).numpy()


def test_class_counts_row_counts_and_k():
    Ks = {r.K for r in sm.ROWS}
    assert Ks == set(sm.KS) | {300} and {1, 2, 3} <= Ks
    for rem in range(4):                                            # every K % 4 on both sides of the 256-element lane stride
        assert any(K % 4 == rem and 4 <= K < 256 for K in Ks) and any(K % 4 == rem and 256 <= K < 512 for K in Ks), rem
    assert {63, 64, 65} <= Ks and 2599 in Ks and any(K % 2 and K > 4 for K in Ks)
    assert {r.rows for r in sm.ROWS} == set(sm.ROW_COUNTS) and any(n % 4 for n in sm.ROW_COUNTS)      # a partial last workgroup
    assert {r.k for r in sm.ROWS} == set(sm.KTOP) == set(range(1, 9))
    for k in sm.KTOP:                                               # every instantiation on several class counts, both sides of 64 and 256
        at = {r.K for r in sm.ROWS if r.k == k and r.law in sm.FINITE_LAWS}
        assert min(at) < 64 and max(at) > 256 and len(at) >= 8, (k, sorted(at))
    assert sum(r.K < r.k for r in sm.ROWS) >= 8                    # K < k: padded with (-1, 0)
    assert {r.K for r in sm.ROWS if r.law == "gauss3"} == set(sm.KS) and all(r.rows == sm.MANY for r in sm.ROWS if r.law == "gauss3")
    for law in ("gauss0.1", "gauss12", "offset+1e4", "offset-1e4", "ascending", "descending"):
        assert {r.K for r in sm.ROWS if r.law == law} >= set(sm.KS), law
    assert 1e6 <= sum(r.rows * r.K for r in sm.ROWS) <= 4e6


def test_every_law_and_mask_placement_occurs():
    assert {r.law for r in sm.ROWS} == set(sm.FINITE_LAWS + sm.MASK_LAWS + sm.POISON_LAWS)
    for r in sm.ROWS:
        x, K4 = sm.row_logits(r), r.K & ~3
        assert x.shape == (r.rows, r.K) and x.dtype == np.float32
        neg, am = np.isneginf(x), x.argmax(axis=1)
        if r.law in sm.FINITE_LAWS:
            assert np.isfinite(x).all()
        if r.law == "ascending":
            assert (np.diff(x, axis=1) > 0).all()                   # every element a lane meets is a new maximum
        elif r.law == "descending":
            assert (np.diff(x, axis=1) < 0).all()
        elif r.law == "max_last_vector":
            assert ((am >= K4 - 4) & (am < K4)).all()
        elif r.law == "max_tail":
            assert (am >= K4).all()
        elif r.law == "max_tied":
            assert ((x == x.max(axis=1, keepdims=True)).sum(axis=1) == len({0, r.K // 2, r.K - 1})).all()
        elif r.law == "mask_index0":
            assert neg[:, 0].all() and neg.sum() == r.rows
        elif r.law == "mask_lane_first":                            # the first element of every lane that has a vector
            assert neg[:, 0:min(K4, 256):4].all() and neg.sum() == r.rows * len(range(0, min(K4, 256), 4))
        elif r.law == "mask_lane_vector":
            assert neg[:, 0:4].all() and not neg[:, 4:8].any()
        elif r.law == "mask_tail":
            keep = K4 if K4 else r.K - 1                            # (K < 4: the row is all tail, its last class is masked)
            assert neg[:, keep:].all() and not neg[:, :keep].any()
        elif r.law == "mask_first256":                              # K <= 300: lanes 4 (K - 256) / 4 .. 63 see -Inf alone
            assert neg[:, :256].all() and not neg[:, 256:].any() and r.K <= 300
        elif r.law == "mask_all_but_one":
            assert (np.isfinite(x).sum(axis=1) == 1).all()
        elif r.law == "mask_all":
            assert neg.all()
        elif r.law == "nan_one":
            assert (np.isnan(x).sum(axis=1) == 1).all()
        elif r.law == "posinf_one":
            assert (np.isposinf(x).sum(axis=1) == 1).all()
        elif r.law == "nan_lane":
            assert r.K == 300 and np.isnan(x[:, 80:84]).all() and np.isnan(x).sum() == 4 * r.rows
    # the lane-stride placements sit where whole lanes are affected: K <= 3 rows are all tail, a NaN there is a lane's only element
    assert {1, 2, 3} <= {r.K for r in sm.ROWS if r.law == "nan_one"} and any(r.K == 300 for r in sm.ROWS if r.law == "mask_first256")
    for law in sm.MASK_LAWS[:4] + sm.MASK_LAWS[5:]:
        assert len({r.K for r in sm.ROWS if r.law == law}) >= 10, law


def test_positions_below_the_normal_range_are_capped():
    """From the float64 oracle alone: posteriors below 2^-126 (where the relative bar gives way to 0 <= got <= 2^-125) are at most
    1 / 8 of a row named deep/..., and there are none in any other row."""
    deep = 0
    for r in sm.ROWS:
        n = topk_oracle.softmax_subnormal(sm.row_logits(r)).sum(axis=1)
        if r.law == "deep":
            assert r.id.startswith("deep/") and (n <= r.K // sm.DEEP_SHARE).all() and (n > 0).all(), (r.id, n)
            deep += int(n.sum())
        else:
            assert not n.any(), (r.id, n)
    assert deep > 1000


@pytest.fixture(scope="module")
def calibration():
    """Per evaluation, (largest softmax_units figure, row) over every row of the matrix."""
    evals = {"numpy": sm.two_pass_f32, "aten": aten_f32, "kernel_order": sm.kernel_order, "serial": sm.serial_f32}
    worst = {name: (0.0, "") for name in evals}
    for r in sm.ROWS:
        x = sm.row_logits(r)
        for name, f in evals.items():
            worst[name] = max(worst[name], (float(topk_oracle.softmax_units(f(x), x).max()), r.id))
    return worst


def test_k_softmax_is_twice_the_float32_evaluations(calibration):
    """K_SOFTMAX is the smallest power of two at or above twice what a plain float32 evaluation reaches: numpy's two-pass softmax
    and ATen's torch.softmax, over every row.  Both have the oracle's classes on every row (a class mismatch is an infinite figure)
    and are inside the bar; so is the kernels' order of operations with a correctly rounded exp.  The strictly serial float32 sum
    is a correct evaluation that the bar REJECTS, by design: the bar separates summation orders (informational, printed)."""
    for name, (u, where) in calibration.items():
        print(f"{name}: max u = {u:.3f} at {where}")
    plain = max(calibration["numpy"][0], calibration["aten"][0])
    assert np.isfinite(plain) and K_SOFTMAX == pow2_at_or_above(2.0 * plain), calibration
    assert calibration["numpy"][0] <= K_SOFTMAX and calibration["aten"][0] <= K_SOFTMAX
    assert calibration["kernel_order"][0] <= K_SOFTMAX / 2, calibration["kernel_order"]
    assert np.isfinite(calibration["serial"][0])


@pytest.mark.parametrize("name", sorted(sm.CONTROL_ROWS))
def test_control_emulations_miss_the_bar(name):
    """The kernels' order of operations with one defect each, on every row of the matrix row named for it: the K % 4 tail classes
    left out of the denominator (a flat 2599-class row: about 1e-3 relative, which no absolute bar sees), one lane's partial sum
    added without its rescale (spread 12), the exponent's argument on a 2^-16 grid."""
    r = sm.control_row(name)
    x = sm.row_logits(r)
    kw = {"tail_dropped": dict(drop_tail=True), "lane_unscaled": dict(unscaled_lane=True), "coarse_argument": dict(grid=2.0 ** -16)}[name]
    clean = topk_oracle.softmax_units(sm.kernel_order(x), x).max(axis=1)
    u = topk_oracle.softmax_units(sm.kernel_order(x, **kw), x).max(axis=1)
    print(name, r.id, "clean", float(clean.max()), "defect", float(u.min()), "..", float(u.max()))
    assert (clean <= K_SOFTMAX).all() and (u >= CONTROL_MARGIN * K_SOFTMAX).all(), (clean, u)
    # what the absolute bars saw of it: the tail's share of a flat row is far below 1e-6 per class
    if name == "tail_dropped":
        assert r.K % 4 == 3 and np.abs(sm.kernel_order(x, **kw).astype(np.float64) - topk_oracle.softmax_f64(x)).max() < 1e-6


def test_the_unguarded_accumulation_turns_a_masked_row_into_nan():
    """What the guard in both kernels' accumulation is for: `if (v > mx) ...; s += exp(v - mx)` on a lane whose first element is
    -Inf computes exp(-Inf - -Inf).  The oracle (and torch) give 0 for the masked class and finite posteriors elsewhere."""
    x = sm.row_logits(next(r for r in sm.ROWS if r.id.startswith("mask_index0/K257")))
    with np.errstate(all="ignore"):
        mx, s = np.float32(-np.inf), np.float32(0)
        for v in x[0, 0:4]:                                          # lane 0's first vector, without the guard
            if v > mx:
                s, mx = s * np.exp(mx - v), v
            s = s + np.exp(v - mx)
    assert np.isnan(s)
    p = topk_oracle.softmax_f64(x)
    assert (p[:, 0] == 0).all() and np.isfinite(p).all() and np.array_equal(np.isnan(aten_f32(x)), np.isnan(p))
    assert float(topk_oracle.softmax_units(sm.kernel_order(x), x).max()) <= K_SOFTMAX


def test_topk_f64_order_and_padding():
    """softmax_topk_f64 against the float32 oracle that the torch goldens pin (finite rows: same indices, probabilities within the
    bar), and its rules for what torch's topk leaves open: masked classes after the finite ones by ascending index, NaN never
    selected, (-1, 0) padding."""
    for r in sm.ROWS:
        x = sm.row_logits(r)
        p, i = topk_oracle.softmax_topk_f64(x, r.k)
        assert p.shape == i.shape == (r.rows, r.k) and ((i >= -1) & (i < r.K)).all()
        n = min(r.k, r.K)
        if r.law not in sm.NAN_ROW_LAWS:
            rp, ri = topk_oracle.softmax_topk(x, n)
            assert np.array_equal(i[:, :n], ri), r.id
            assert float(topk_oracle.softmax_units(rp, x, i[:, :n]).max()) <= K_SOFTMAX, r.id
            assert (i[:, n:] == -1).all() and (p[:, n:] == 0).all()
            lg = np.take_along_axis(x, i[:, :n], axis=1)
            assert (lg[:, 1:] <= lg[:, :-1]).all() and (i[:, 1:n] > i[:, :n - 1])[lg[:, 1:] == lg[:, :-1]].all()
    x = np.array([[1.0, -np.inf, 3.0, -np.inf, 2.0], [np.nan, 1.0, 2.0, np.nan, -np.inf]], np.float32)
    p, i = topk_oracle.softmax_topk_f64(x, 6)
    assert i.tolist() == [[2, 4, 0, 1, 3, -1], [2, 1, 4, -1, -1, -1]]
    assert (p[0, 3:] == 0).all() and np.isnan(p[1, :3]).all() and (p[1, 3:] == 0).all()


def test_softmax_units_put_classes_first():
    x = np.array([[0.0, 1.0, -np.inf, 2.0]], np.float32)
    p = topk_oracle.softmax_f64(x).astype(np.float32)
    assert topk_oracle.softmax_units(p, x).max() <= 1.0
    assert topk_oracle.softmax_units(np.zeros((1, 4), np.float32), x)[0, 0] > 1e6          # an all-zero output: finite, far outside
    for pos, bad in ((2, 1e-30), (2, np.nan), (0, np.nan), (1, np.inf)):
        q = p.copy()
        q[0, pos] = bad
        assert np.isinf(topk_oracle.softmax_units(q, x)[0, pos]), (pos, bad)
    assert np.isinf(topk_oracle.softmax_units(np.zeros((1, 4), np.float32), np.full((1, 4), -np.inf, np.float32))).all()
    deep = np.array([[0.0, -100.0]], np.float32)                   # below the normal range: flushing allowed, nothing above 2^-125
    assert topk_oracle.softmax_units(np.array([[1.0, 0.0]], np.float32), deep).max() == 0.0
    assert np.isinf(topk_oracle.softmax_units(np.array([[1.0, 1e-37]], np.float32), deep)[0, 1])


def test_the_hook_is_in_the_hooks_library_alone():
    hooks, product = C.CDLL(hooks_path()), C.CDLL(_capi.lib_path())
    assert hasattr(hooks, "wekws_hip_debug_softmax_rows") and not hasattr(product, "wekws_hip_debug_softmax_rows")
