"""CPU: the float64 oracle of the criterion (tests/criterion_ref.py) against what the live reference returned
(tests/golden/criterion_golden.npz), the bars' derivation, a negative control, and the executor's running totals."""
import os

import numpy as np
import pytest
import torch

from tests import criterion_matrix as cm
from tests import criterion_ref as cr
from tests.helpers import pow2_at_or_above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "criterion_golden.npz"))


def test_bars_follow_from_the_reference_error(gold):
    for kind, bar in cm.BARS.items():
        ref = float(gold[kind + "/ref_units"])
        assert abs(ref - cm.REF_UNITS[kind]) < 0.01, (kind, ref)
        assert bar == pow2_at_or_above(4 * ref), (kind, ref, bar)


@pytest.mark.parametrize("name", cm.case_names("max_pooling"))
def test_max_pooling_oracle_matches_the_reference(gold, name):
    c = cm.load_case("max_pooling", name, gold)
    o = cr.max_pooling(**c)
    assert np.array_equal(o["pooled"], gold[name + "/pooled"], equal_nan=True)
    assert np.array_equal(o["correct"], gold[name + "/correct"])
    assert o["acc"] == float(gold[name + "/acc"])
    assert cm.units(gold[name + "/loss"], o["loss"]) <= cm.BARS["max_pooling"]


def test_max_pooling_cases_cover_the_edges():
    names = cm.case_names("max_pooling")
    cases = [cm.max_pooling_case(n) for n in names]
    lens = np.concatenate([c["lengths"] for c in cases])
    assert {0, 1}.issubset(set(lens.tolist())) and all(c["lengths"].max() == c["scores"].shape[1] for c in cases)
    assert {0, 5}.issubset({c["min_duration"] for c in cases})
    assert any(c["min_duration"] > c["lengths"][c["lengths"] > 0].min() for c in cases)
    c = cm.max_pooling_case("mp_5x37x3_md0")
    assert set(c["target"].tolist()) == {-1, 0, 1, 2, 3} and (c["scores"] == 0.5).any()
    c = cm.max_pooling_case("mp_5x37x3_nan")
    nan_t = np.argwhere(np.isnan(c["scores"]))
    assert any(t < c["lengths"][b] for b, t, _ in nan_t) and any(t >= c["lengths"][b] for b, t, _ in nan_t)


@pytest.mark.parametrize("name", cm.case_names("ce"))
def test_cross_entropy_oracle_matches_the_reference(gold, name):
    c = cm.load_case("ce", name, gold)
    o = cr.cross_entropy(**c)
    assert np.array_equal(o["pred"], gold[name + "/pred"])
    assert o["acc"] == float(gold[name + "/acc"])
    assert cm.units(gold[name + "/loss"], o["loss"]) <= cm.BARS["ce"]


@pytest.mark.parametrize("name", cm.case_names("ctc"))
def test_ctc_oracle_matches_the_reference(gold, name):
    c = cm.load_case("ctc", name, gold)
    o = cr.ctc(**c)
    assert cm.units(gold[name + "/rows"], o["rows"]) <= cm.BARS["ctc"]         # +Inf rows: the class must match
    assert cm.units(gold[name + "/loss"], o["loss"]) <= cm.BARS["ctc"]


def test_ctc_cases_hold_repeats_and_an_infeasible_row(gold):
    """The wrong recursion -- the skip transition between EQUAL labels too -- must miss the goldens: the cases contain
    adjacent repeats, and the infeasible row is infeasible only because of them."""
    missed = 0
    for name in cm.case_names("ctc"):
        c = cm.load_case("ctc", name, gold)
        rows = gold[name + "/rows"]
        wrong = cr.ctc(**c, skip_equal_labels=True)["rows"]
        if cm.units(rows, wrong) > cm.BARS["ctc"]:
            missed += 1
    assert missed >= 3
    c = cm.load_case("ctc", "ctc_v7_t50", gold)
    assert np.isinf(gold["ctc_v7_t50/rows"][5]) and np.isfinite(cr.ctc(**c, skip_equal_labels=True)["rows"][5])
    assert np.isinf(gold["ctc_v7_t1/rows"][2])


@pytest.mark.parametrize("name", cm.case_names("acc"))
def test_utterance_accuracy_oracle_matches_the_reference(gold, name):
    c = cm.load_case("acc", name, gold)
    o = cr.utterance_accuracy(**c)
    assert np.array_equal(o["dist"], gold[name + "/dist"])
    assert [o["words"], o["errors"]] == gold[name + "/totals"].tolist()
    assert o["acc"] == float(gold[name + "/acc"])
    assert (c["target_lengths"] == 0).any() and (gold[name + "/dist"] > 0).any()
    assert cm.units(gold[name + "/loss"], cr.ctc(**c)["loss"]) <= cm.BARS["ctc"]
    empty = dict(c, target_lengths=np.zeros_like(c["target_lengths"]))
    with pytest.raises(ZeroDivisionError):
        cr.utterance_accuracy(**empty)


def test_edit_distance():
    assert cr.edit_distance([], []) == 0 and cr.edit_distance([1, 2], []) == 2 and cr.edit_distance([], [3]) == 1
    assert cr.edit_distance([1, 2, 3], [1, 3]) == 1 and cr.edit_distance([1, 2, 3], [4, 2, 5, 6]) == 3
    rng = np.random.default_rng(0)
    for _ in range(50):
        a, b = rng.integers(1, 4, rng.integers(0, 8)).tolist(), rng.integers(1, 4, rng.integers(0, 8)).tolist()
        assert cr.edit_distance(a, b) == cr.edit_distance(b, a) <= max(len(a), len(b))


def test_executor_totals_equal_the_host_loop_bit_for_bit(gold):
    """RunningTotals (what Executor.cv keeps on the device) on recorded per-batch values -- the goldens' losses and
    accuracies, non-finite ones included -- against the restated host loop."""
    from wekws_amd.utils.executor import RunningTotals
    batches = []
    for kind in ("max_pooling", "ce", "acc"):
        for i, name in enumerate(cm.case_names(kind)):
            batches.append((np.float32(gold[name + "/loss"]), float(gold[name + "/acc"]), 3 + 7 * i))
    batches.append((np.float32(np.inf), 50.0, 9))
    assert any(not np.isfinite(b[0]) for b in batches[:-1])          # the NaN batch of mp_5x37x3_nan
    tot = RunningTotals("cpu")
    for loss, acc, n in batches:
        tot.add(torch.tensor(loss), torch.tensor(acc, dtype=torch.float64), n)
    got = tot.result()
    want = cr.executor_loop(batches)
    assert np.array_equal(np.array(got).view(np.int64), np.array(want).view(np.int64)), (got, want)
    assert int(tot.num_seen_utts) == 1 + sum(n for l, _, n in batches if np.isfinite(l))
    tot.add(torch.tensor(1.0), torch.tensor(float("nan"), dtype=torch.float64), 2)      # an accuracy the reference cannot compute
    with pytest.raises(ZeroDivisionError):
        tot.result()


def test_criterion_refuses_cpu_tensors_and_unknown_kinds():
    from wekws_amd import criterion as crit
    from wekws_amd.utils.executor import Executor
    with pytest.raises(ValueError, match="no CPU fallback"):
        crit.criterion("max_pooling", torch.zeros(1, 2, 1), torch.zeros(1), torch.ones(1))
    with pytest.raises(ValueError, match="no CPU fallback"):
        crit.criterion("ce", torch.zeros(1, 2), torch.zeros(1), None)
    with pytest.raises(ValueError, match="no CPU fallback"):
        crit.criterion("ctc", torch.zeros(1, 2, 3), torch.zeros(1, 1), torch.ones(1), torch.ones(1))
    with pytest.raises(ValueError, match="unknown criterion"):
        crit.criterion("mse", torch.zeros(1, 2), torch.zeros(1), None)
    with pytest.raises(NotImplementedError):
        Executor().train(None, None, [], "cpu", None, {})


def test_argument_errors_return_einval_and_launch_nothing():
    from wekws_amd import _capi
    lib = _capi.load()
    p = 4096                                                         # any non-NULL value: nothing is dereferenced
    assert lib.wekws_hip_criterion_max_pooling(None, 1, 1, 1, p, p, 0, p, p, p, p, p, None) == -1 and "NULL" in _capi.last_error()
    assert lib.wekws_hip_criterion_max_pooling(p, -1, 1, 1, p, p, 0, p, p, p, p, p, None) == -1 and "B=-1" in _capi.last_error()
    assert lib.wekws_hip_criterion_ce(p, 1, 2, None, p, p, p, p, p, None) == -1
    assert lib.wekws_hip_criterion_ce(p, 1, -2, p, p, p, p, p, p, None) == -1 and "D=-2" in _capi.last_error()
    assert lib.wekws_hip_ctc_loss_workspace_bytes(3, 5, 7) == 3 * 5 * 8 * 4 and lib.wekws_hip_ctc_loss_workspace_bytes(-1, 5, 7) == 0
    assert lib.wekws_hip_ctc_loss(p, 1, 1, 2, p, 1, p, p, p, p, None, None, 64, None) == -1 and "NULL" in _capi.last_error()
    assert lib.wekws_hip_ctc_loss(p, 1, 1, 2, p, -1, p, p, p, p, None, p, 64, None) == -1 and "Lmax=-1" in _capi.last_error()
    assert lib.wekws_hip_ctc_loss(p, 2, 5, 2, p, 3, p, p, p, p, None, p, 8, None) == -1 and "workspace" in _capi.last_error()
    assert lib.wekws_hip_ctc_edit_distance(None, 5, 10, 1, p, 1, p, p, None, None) == -1
    assert lib.wekws_hip_ctc_edit_distance(p, 5, 10, -1, p, 1, p, p, None, None) == -1 and "B=-1" in _capi.last_error()
