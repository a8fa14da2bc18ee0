"""CPU: the float64 oracle of the criterion's gradient (tests/criterion_grad_ref.py) against what torch's autograd gave for the
live reference (tests/golden/criterion_grad_golden.npz), the tie and clamp rules against hand values, the bars' derivation,
and the argument checks of the C entry points."""
import os

import numpy as np
import pytest

from tests import criterion_grad_matrix as gm
from tests import criterion_grad_ref as gr
from tests.helpers import pow2_at_or_above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(k, n) for k in ("max_pooling", "ce", "ctc") for n in gm.case_names(k)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "criterion_grad_golden.npz"))


def oracle(kind, c, divisor, upstream=1.0):
    """-> (gradient float64, per-row nll float64 or None)"""
    if kind == "max_pooling":
        return gr.max_pooling_grad(c["scores"], c["target"], c["lengths"], c["min_duration"], upstream, divisor), None
    if kind == "ce":
        return gr.cross_entropy_grad(c["logits"], c["target"], upstream, divisor), None
    o = gr.ctc_grad(c["logits"], c["targets"], c["lengths"], c["target_lengths"], upstream, divisor)
    return o["grad"], o["rows"]


def golden_classes(gold, name, shape):
    n = int(np.prod(shape))
    nan = np.unpackbits(gold[name + "/nan32"])[:n].astype(bool)
    zero = np.unpackbits(gold[name + "/zero32"])[:n].astype(bool)
    return np.where(nan, 2, np.where(zero, 1, 0)).astype(np.uint8).reshape(shape)


def deviation(kind, got, ref, divisor, rows, where=None):
    """max |got - ref| / max(|ref|, scale) over the elements of equal class; scale: the units' denominators."""
    same = gm.classes(got) == gm.classes(ref)
    if where is not None:
        same = same & where
    fin = same & np.isfinite(ref)
    scale = np.full(ref.shape, 1.0 / divisor)
    if kind == "ctc":
        nll = np.where(np.isfinite(rows), np.maximum(1.0, rows), 1.0)
        scale = scale * nll.reshape((-1,) + (1,) * (ref.ndim - 1))
    return float((np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)) / np.maximum(np.where(fin, np.abs(ref), 0.0), scale)).max())


@pytest.mark.parametrize("kind,name", CASES)
def test_oracle_matches_the_reference_autograd(gold, kind, name):
    c = gm.load_case(kind, name)
    B = gm.batch_size(kind, c)
    o, rows = oracle(kind, c, B)
    # classes: exactly those of the reference's float32 gradient
    assert np.array_equal(gm.classes(o), golden_classes(gold, name, o.shape))
    if name + "/grad64" in gold.files:
        g64 = gold[name + "/grad64"]
        if kind == "max_pooling":        # float64 autograd decides ties and gates on other numbers: compared where the classes agree
            kw = gm.keyword_columns(c)
            assert deviation(kind, o, g64, B, rows, kw) <= 1e-12
            assert deviation(kind, o, g64, B, rows, ~kw) <= gm.MP_OTHER_TOL
            assert (gm.classes(g64) != gm.classes(o)).sum() <= 1
        else:
            assert np.array_equal(gm.classes(o), gm.classes(g64))
            assert deviation(kind, o, g64, B, rows) <= 1e-12
    else:
        assert float(gold[name + "/oracle_dev"]) <= 1e-12
        s = float(gold[name + "/grad64_sum"])
        mine = float(o[np.isfinite(o)].sum())
        assert abs(mine - s) <= 1e-12 * max(1.0, float(np.abs(o[np.isfinite(o)]).sum()))
    if rows is not None:
        r64 = gold[name + "/rows64"]
        assert np.array_equal(gm.classes(rows), gm.classes(r64))
        fin = np.isfinite(r64)
        assert np.allclose(rows[fin], r64[fin], rtol=1e-12, atol=1e-12)


def test_ties_and_the_clamp_gate_by_hand():
    c = gm.load_case("max_pooling", "mpg_ties_6x4x2")
    g = gr.max_pooling_grad(**c)
    p7, one = float(np.float32(0.7)), 1.0
    assert np.allclose(g[0, :, 0], [0, -(one / p7) / 2, -(one / p7) / 2, 0], rtol=1e-15, atol=0)
    assert np.allclose(g[0, :, 0], gm.TIE_HAND, rtol=1e-15, atol=0) and abs(g[0, 1, 0] + 0.714285) < 1e-6
    q = float(np.float32(1.0) - np.float32(0.6))
    assert np.allclose(g[0, :, 1], [0, (one / q) / 2, (one / q) / 2, 0], rtol=1e-15, atol=0)
    assert g[1, :, 0].tolist() == [0, 0, -0.5, 0]                    # 1.25 wins with 1.0: the gate lets only the 1.0 through
    assert g[2, :, 0].tolist() == [0, -1.0, 0, 0]                    # a score of exactly 1.0 receives -1
    assert g[2, :, 1].tolist() == [0.25, 0, 0.25, 0.25]              # 1 - x == 1 passes (inclusive), 1 - x == 1.25 does not
    assert np.allclose(g[3, :, 0], [-(one / float(np.float32(1e-8))) / 4, 0, 0, 0], rtol=1e-15, atol=0)    # x == float32(1e-8): inclusive
    assert not g[3, :, 1].any()                                      # 1 - x == 0 wins clamped to 1e-8 and fails the gate
    assert np.count_nonzero(g[4, :, 1]) == 2 and g[4, 3, 1] == 0 and g[4, 0, 1] == g[4, 1, 1] > 0       # filler row, tie inside the length
    assert np.count_nonzero(g[5, :, 0]) == 2 and not g[5, 2:, 0].any()
    c = gm.load_case("max_pooling", "mpg_masked_3x6x2")
    g = gr.max_pooling_grad(**c)
    assert not g[0, :, 0].any() and g[0, :, 1].any() and not g[2].any()        # min_duration >= len: T ties at 1e-8, all gated
    c = gm.load_case("max_pooling", "mp_5x37x3_nan")
    g = gr.max_pooling_grad(**c)
    assert not np.isnan(g).any() and not g[0, :, 1].any() and not g[4, :, 2].any()     # a NaN pooled value: zeros


def test_divisor_and_upstream_scale_the_oracle():
    for kind, name in (("max_pooling", "mpg_ties_6x4x2"), ("ce", "ce_7x12"), ("ctc", "ctcg_v12_t9")):
        c = gm.load_case(kind, name)
        B = gm.batch_size(kind, c)
        g1, _ = oracle(kind, c, 1)
        gb, _ = oracle(kind, c, B, 2.0)
        assert np.allclose(gb, g1 * 2.0 / B, rtol=1e-15, atol=0, equal_nan=True)


def test_ctc_cases_reach_repeats_and_the_global_frames():
    c = gm.load_case("ctc", "ctcg_v12_t9")
    assert c["targets"][0, :3].tolist() == [4, 9, 4] and c["targets"][1].tolist() == [4, 4, 9, 4]
    o = gr.ctc_grad(**c)
    assert np.isfinite(o["rows"]).all() and not o["grad"][2, 5:].any()
    assert np.abs(o["grad"][:, :, :].sum(axis=2)).max() < 1e-12         # softmax and the occupancies both sum to 1
    c = gm.load_case("ctc", "ctcg_v5_t560")
    assert 2 * c["targets"].shape[1] + 1 > gm.CTC_LDS_STATES >= 2 * 128 + 1
    src = open(os.path.join(ROOT, "wekws_amd", "csrc", "criterion_grad.hip.h")).read()
    assert f"kCtcGradLdsStates = {gm.CTC_LDS_STATES};" in src
    for name in ("ctc_v7_t1", "ctc_v7_t50"):                            # the infeasible rows: NaN on the valid frames, 0 beyond
        c = gm.load_case("ctc", name)
        o = gr.ctc_grad(**c)
        for b in np.flatnonzero(np.isinf(o["rows"])):
            n = int(c["lengths"][b])
            assert np.isnan(o["grad"][b, :n]).all() and not o["grad"][b, n:].any()


def test_bars_follow_from_the_reference_error(gold):
    for kind, bar in gm.BARS.items():
        ref = float(gold[kind + "/ref_units"])
        assert abs(ref - gm.REF_UNITS[kind]) < 0.01, (kind, ref)
        assert bar == pow2_at_or_above(4 * ref), (kind, ref, bar)


def test_units_see_a_class_change_and_an_error():
    c = gm.load_case("ctc", "ctc_v7_t50")
    o = gr.ctc_grad(**c, divisor=9)
    g = o["grad"].copy()
    assert gm.units("ctc", g, o["grad"], 9, o["rows"]) == 0.0
    g[0, 0, 0] += 2.0 ** -24 * max(1.0, o["rows"][0]) / 9 * 3
    assert abs(gm.units("ctc", g, o["grad"], 9, o["rows"]) - 3.0) < 1e-6
    g[3, 40, 0] = 1e-30                                                  # a frame beyond the length must be exactly 0
    assert gm.units("ctc", g, o["grad"], 9, o["rows"]) == float("inf")


def test_argument_errors_return_einval_and_launch_nothing():
    from wekws_amd import _capi
    lib = _capi.load()
    p = 4096                                                         # any non-NULL value: nothing is dereferenced
    mp, ce, ctc = lib.wekws_hip_criterion_max_pooling_grad, lib.wekws_hip_criterion_ce_grad, lib.wekws_hip_ctc_loss_grad
    assert mp(None, 1, 1, 1, p, p, 0, None, 1, p, None) == -1 and "NULL" in _capi.last_error()
    assert mp(p, 1, 1, 1, p, p, 0, None, 1, None, None) == -1 and "NULL" in _capi.last_error()
    assert mp(p, -1, 1, 1, p, p, 0, None, 1, p, None) == -1 and "B=-1" in _capi.last_error()
    assert mp(p, 1, 1, 1, p, p, 0, None, 0, p, None) == -1 and "divisor=0" in _capi.last_error()
    assert ce(p, 1, 2, None, None, 1, p, None) == -1 and "NULL" in _capi.last_error()
    assert ce(p, 1, -2, p, None, 1, p, None) == -1 and "D=-2" in _capi.last_error()
    assert ce(p, 1, 2, p, None, -3, p, None) == -1 and "divisor=-3" in _capi.last_error()
    need = lib.wekws_hip_ctc_loss_grad_workspace_bytes(2, 5, 3)
    # the alphas / occupancies and the beta ping-pong in double, the row's nll, the forward's lp, two statistics a frame, the links
    assert need == (2 * 5 * 7 * 8 + 2 * 2 * 7 * 8 + 2 * 8 + 2 * 5 * 4 * 4 + 2 * 5 * 2 * 4 + 2 * 2 * 3 * 4 + 15) // 16 * 16
    assert need >= lib.wekws_hip_ctc_loss_workspace_bytes(2, 5, 3) and lib.wekws_hip_ctc_loss_grad_workspace_bytes(-1, 5, 7) == 0
    assert ctc(p, 2, 5, 2, p, 3, p, p, None, 1, p, p, None, p, need, None) == -1 and "NULL" in _capi.last_error()
    assert ctc(p, 2, 5, 2, p, 3, p, p, None, 1, p, p, p, None, need, None) == -1 and "NULL" in _capi.last_error()
    assert ctc(p, 2, 5, 2, p, -1, p, p, None, 1, p, p, p, p, need, None) == -1 and "Lmax=-1" in _capi.last_error()
    assert ctc(p, 2, 5, 2, p, 3001, p, p, None, 1, p, p, p, p, 1 << 40, None) == -1 and "Lmax=3001" in _capi.last_error()
    assert ctc(p, 2, 5, 2, p, 3, p, p, None, 0, p, p, p, p, need, None) == -1 and "divisor=0" in _capi.last_error()
    assert ctc(p, 2, 5, 2, p, 3, p, p, None, 1, p, p, p, p, need - 1, None) == -1 and "workspace" in _capi.last_error()
    assert ctc(p, 2, 5, 2, p, 3, p, p, None, 1, p, p, p, p + 4, need, None) == -1 and "aligned" in _capi.last_error()


def test_executor_train_still_refuses_and_train_executor_exists():
    from wekws_amd.utils.executor import Executor, TrainExecutor
    with pytest.raises(NotImplementedError, match="TrainExecutor"):
        Executor().train(None, None, [], "cpu", None, {})
    assert issubclass(TrainExecutor, Executor) and TrainExecutor.train is not Executor.train
    assert TrainExecutor.cv is Executor.cv
