"""Case list, units and bars of the criterion-gradient tests (tests/test_criterion_grad_oracle.py on the CPU,
tests/test_hip_criterion_grad.py on the GPU; goldens: tests/golden/make_criterion_grad_golden.py -> criterion_grad_golden.npz
from the live wekws.model.loss.criterion under torch's autograd).

Cases: every case of tests/criterion_matrix.py (max_pooling, ce, ctc and the acc inputs as ctc), plus small ones that reach
what those do not:

    mpg_ties_6x4x2     two equal maxima in a keyword column ([0.3, 0.7, 0.7, 0.2] -> [0, -1/0.7/2, -1/0.7/2, 0]) and two equal
                       minima in another column; a winning score above 1 beside one of exactly 1.0 (the first gets 0, the second
                       -1/2); a lone winner of exactly 1.0 (-1); a keyword score of exactly float32(1e-8) tied with three clamped
                       frames (-(1 / 1e-8) / 4 on it alone); another column at x = 0 and below (1 - x = 1 ties, the gate's
                       inclusive upper end; 1 - x = 1.25 gets 0); another column holding x = 1 (1 - x = 0 is clamped to 1e-8,
                       wins the minimum and fails the gate: all zeros)
    mpg_masked_3x6x2   min_duration (4) >= the length (3, 0) of a keyword row: all T frames tie at 1e-8, every gradient is 0
    ctcg_v12_t9        labels [4, 9, 4] (one class in two non-adjacent states), [4, 4, 9, 4], [9], a length below T
    ctcg_v5_t560       520 labels: 1041 extended states, beyond the 1024 up to which the alpha-beta kernel keeps its frames in
                       LDS; a second row of 100 labels and 300 frames

`1 - x` of exactly 1e-8 does not exist in float32 (below 1 the spacing is 2^-24 = 6e-8), so the lower end of that gate is met
from outside (x = 1) and on the keyword column, where x = float32(1e-8) is representable.

Units (`units(kind, ...)`), after the classes (NaN, exact 0) have matched exactly:

    max_pooling, ce   per element   |got - ref64| / (2^-24 * max(1 / divisor, |ref64|))
    ctc               per row       max|got - ref64| / (2^-24 * max(1, nll_row) / divisor)   (the exponentiated log-domain sums
                                    have the magnitude of the row's loss; rows without a finite loss: classes only)

BARS -- the project's rule (tests/criterion_matrix.py): pow2_at_or_above(4 x the worst units of the reference's own float32
gradient -- torch's autograd on the CPU -- against the float64 oracle, tests/criterion_grad_ref.py, over this matrix).
Measured by make_criterion_grad_golden.py (printed there, stored as <kind>/ref_units, checked on the CPU):

    kind          reference's worst units          bar    device's worst units (MI355X)
    max_pooling   1.37  (mp_300x3x2_md0)             8      1.64 (mp_300x3x2_md0)
    ce            5.61  (ce_300x2599)                32     2.80 (ce_300x2599)
    ctc           15.80 (ctcg_v5_t560)               64     3.11 (acc_v16_t30)
"""
from __future__ import annotations

import numpy as np

from tests import criterion_matrix as cm

SMALL = cm.SMALL
REF_UNITS = {"max_pooling": 1.37, "ce": 5.61, "ctc": 15.8}          # measured: <kind>/ref_units of the golden file
BARS = {"max_pooling": 8.0, "ce": 32.0, "ctc": 64.0}               # pow2_at_or_above(4 x REF_UNITS)
CTC_LDS_STATES = 1024                                             # wekws::kCtcGradLdsStates


def classes(a):
    """0 finite and non-zero, 1 exactly zero, 2 NaN, 3 infinite."""
    a = np.asarray(a)
    return np.where(np.isnan(a), 2, np.where(np.isinf(a), 3, np.where(a == 0, 1, 0))).astype(np.uint8)


def units(kind, got, ref64, divisor, nll_rows=None):
    """Worst error in the unit of the bars; inf when a class (NaN / exact zero / finite) differs."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref64, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.array_equal(classes(got), classes(ref)):
        return float("inf")
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    err = np.where(fin, np.abs(got - np.where(fin, ref, 0.0)), 0.0)
    if kind == "ctc":
        nll = np.asarray(nll_rows, np.float64)
        worst = 0.0
        for b in range(ref.shape[0]):
            if np.isfinite(nll[b]):
                worst = max(worst, float(err[b].max()) / (2.0 ** -24 * max(1.0, nll[b]) / divisor))
        return worst
    return float((err / (2.0 ** -24 * np.maximum(1.0 / divisor, np.where(fin, np.abs(ref), 0.0)))).max())


# ------------------------------------------------------------------------------------------------ max pooling
MAX_POOLING_NEW = ("mpg_ties_6x4x2", "mpg_masked_3x6x2")
TIE_HAND = [0.0, -(1.0 / float(np.float32(0.7))) / 2, -(1.0 / float(np.float32(0.7))) / 2, 0.0]     # row 0, column 0, divisor 1


def max_pooling_case(name):
    if name in cm.MAX_POOLING:
        return cm.max_pooling_case(name)
    if name == "mpg_ties_6x4x2":
        s = np.empty((6, 4, 2), np.float32)
        s[0, :, 0] = [0.3, 0.7, 0.7, 0.2]
        s[0, :, 1] = [0.1, 0.6, 0.6, 0.2]
        s[1, :, 0] = [0.3, 1.25, 1.0, 0.2]
        s[1, :, 1] = [0.5, 0.25, 0.5, 0.125]
        s[2, :, 0] = [0.3, 1.0, 0.2, 0.9]
        s[2, :, 1] = [0.0, -0.25, 0.0, 0.0]
        s[3, :, 0] = [1e-8, 0.0, -0.5, 1e-9]
        s[3, :, 1] = [0.5, 1.0, 0.75, 0.25]
        s[4, :, 0] = [0.25, 0.5, 0.5, 0.5]                      # a filler row: both columns pool the minimum of 1 - x
        s[4, :, 1] = [0.9, 0.9, 0.1, 0.9]                       # the tie at 0.9 reaches into the masked frame 3 (len 3): no tie there
        s[5, :, 0] = [0.4, 0.4, 0.9, 0.9]                       # len 2: the maximum ties inside the length only
        s[5, :, 1] = [0.2, 0.3, 0.3, 0.3]
        return dict(scores=s, target=np.array([0, 0, 0, 0, -1, 0], np.int32), lengths=np.array([4, 4, 4, 4, 3, 2], np.int32),
                    min_duration=0)
    if name == "mpg_masked_3x6x2":
        s = np.random.default_rng(21).random((3, 6, 2), dtype=np.float32)
        return dict(scores=s, target=np.array([0, 1, 1], np.int32), lengths=np.array([3, 6, 0], np.int32), min_duration=4)
    raise KeyError(name)


def keyword_columns(case):
    """(B, T, K) bool: the elements of each row's keyword column."""
    B, T, K = case["scores"].shape
    return np.broadcast_to((np.arange(K)[None, :] == np.asarray(case["target"])[:, None])[:, None, :], (B, T, K))


# The columns that pool 1 - x: the oracle (like tests/criterion_ref.py) takes 1 - x as the ONE float32 subtraction the device and the
# reference's float32 run make; torch's float64 autograd subtracts in float64, so its 1 / Q differs by that rounding, 2^-24 relative.
MP_OTHER_TOL = 2.0 ** -23


# ------------------------------------------------------------------------------------------------ ctc
CTC_NEW = {
    "ctcg_v12_t9": (12, 9, [(9, [4, 9, 4]), (9, [4, 4, 9, 4]), (5, [9]), (7, [4, 9, 4])], 401),
    "ctcg_v5_t560": (5, 560, [(560, "s520"), (300, "s100")], 402),
}


def ctc_case(name):
    if name in cm.CTC:
        return cm.ctc_case(name)
    if name in cm.ACC:
        return cm.acc_case(name)
    V, T, rows, seed = CTC_NEW[name]
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((len(rows), T, V)) * 2).astype(np.float32)
    labs = []
    for _, lab in rows:
        if isinstance(lab, str):
            lab = np.cumsum(rng.integers(1, V - 1, int(lab[1:]))) % (V - 1) + 1     # neighbours differ: the row stays feasible ...
            lab[5:9] = lab[5]                                                        # ... with a few adjacent repeats put back
            lab = lab.tolist()
        labs.append(list(lab))
    Lmax = max(len(l) for l in labs)
    targets = np.zeros((len(rows), Lmax), np.int32)
    for i, l in enumerate(labs):
        targets[i, :len(l)] = l
    return dict(logits=x, targets=targets, lengths=np.array([r[0] for r in rows], np.int32),
                target_lengths=np.array([len(l) for l in labs], np.int32))


KINDS = {
    "max_pooling": (sorted(cm.MAX_POOLING) + list(MAX_POOLING_NEW), max_pooling_case, "scores"),
    "ce": (sorted(cm.CE), cm.ce_case, "logits"),
    "ctc": (sorted(cm.CTC) + sorted(cm.ACC) + sorted(CTC_NEW), ctc_case, "logits"),
}


def case_names(kind):
    return list(KINDS[kind][0])


def load_case(kind, name):
    return KINDS[kind][1](name)


def batch_size(kind, case):
    return int(np.asarray(case[KINDS[kind][2]]).shape[0])
