"""CPU: the oracle of tests/pointwise_conv_ref.py against the live reference's goldens, the bars of tests/pointwise_conv_matrix.py
recomputed, the emulation of the kernels' arithmetic under them and inside the element bounds (the evidence that they can be met
before any GPU run), the negative control, and the plan of csrc/pointwise_conv_plan.h through the C ABI, without a device: equal
to the Linear weight gradient's plan, and every refusal."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import linear_wgrad_matrix as lm
from tests import pointwise_conv_matrix as pm
from tests import pointwise_conv_ref as pr
from tests.helpers import pow2_at_or_above
from wekws_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def one_thread():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                      # the sums' order, and so the recorded units, must not depend on the core count
    yield
    torch.set_num_threads(threads)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "pointwise_conv_golden.npz"))


def _plan(B, Ci, T, Co):
    out = (ctypes.c_int64 * 7)()
    rc = _capi.load().wekws_hip_pointwise_conv1d_plan(B, Ci, T, Co, out)
    return rc, list(out)


def test_matrix_covers_what_it_says():
    K = pm.chain_rows()
    cases = pm.cases()
    shape = lambda s: (s["B"], s["Ci"], s["Co"], s["T"])  # noqa: E731
    assert {s["T"] for s in cases.values() if shape(s)[:3] == (2, 16, 16)} >= {1, 15, 16, 17, 63, 64, 65, 129}
    edge = {1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65}
    sweep = [s for s in cases.values() if (s["B"], s["T"]) == (2, 35)]
    assert {s["Ci"] for s in sweep} >= edge and {s["Co"] for s in sweep} >= edge
    assert shape(cases["ragged"]) == (3, 130, 67, 70) and shape(cases["chain600"]) == (3, 8, 8, 200)
    assert 2 * 200 < K < 3 * 200                                          # the chain boundary falls inside batch row 2
    assert shape(cases["straddle"]) == (5, 4, 4, 103)
    assert [cases[n]["B"] * cases[n]["T"] for n in ("rK-1", "rK", "rK+1", "r2K+1")] == [K - 1, K, K + 1, 2 * K + 1]
    s = cases["slices"]
    p = pm.device_plan(s["B"], s["Ci"], s["T"], s["Co"])
    assert p["slices"] >= 3 and p["chains_per_slice"] >= 2 and (s["B"] * s["T"]) % K != 0          # a ragged last slice
    assert p["chains"] - (p["slices"] - 1) * p["chains_per_slice"] < p["chains_per_slice"]
    assert not cases["nobias"]["bias"] and "db" not in cases["nobias"]["wants"]
    assert [set(cases[n]["wants"]) for n in ("nodx", "nodw", "nodb")] == [{"dw", "db"}, {"dx", "db"}, {"dx", "dw"}]
    assert {s["flavour"] for s in cases.values()} >= {"unaligned", "nan", "inf", "large", "recipe"}
    assert {shape(s) for s in cases.values() if s["flavour"] == "recipe"} == {
        (256, 64, 64, 100), (100, 32, 32, 200), (100, 80, 32, 200), (256, 256, 256, 100)}
    o = pm.oracle("large")
    assert all(np.isfinite(o[q]).all() for q in pm.QUANTITIES) and max(np.abs(o["abs_" + q]).max() for q in pm.QUANTITIES) < 2.0 ** 127
    assert np.abs(pm.load_case("large")["x"]).max() > 2.0 ** 40
    assert set(pm.GOLDEN) <= set(pm.small_case_names())


@pytest.mark.parametrize("name", sorted(pm.GOLDEN))
def test_oracle_against_the_references_golden(golden, name):
    """The seeded inputs are the recorded ones; the float64 oracle is the reference's float64 convolution and autograd to a few
    units of 2^-53, and the reference's float32 run is inside the bars."""
    c, ref = pm.load_case(name), pm.oracle(name)
    for k in ("x", "g", "w", "bias"):
        if c[k] is None:
            assert f"{name}/{k}" not in golden.files
        else:
            assert np.array_equal(c[k], golden[f"{name}/{k}"]), (name, k)
    qs = [q for q in pm.QUANTITIES if c["bias"] is not None or q != "db"]
    for q in qs:
        g64 = golden[f"{name}/{q}64"]
        assert g64.shape == ref[q].shape
        assert np.abs(g64 - ref[q]).max() <= 2.0 ** -40 * np.abs(ref[q]).max(), (name, q)
    u, bad = pm.units(name, {q: golden[f"{name}/{q}32"] for q in qs})
    assert not bad
    for q in qs:
        assert u[q] <= pm.BARS[q], (name, q, u[q])


def _torch_run(c):
    x = torch.from_numpy(c["x"].copy()).requires_grad_()
    w = torch.from_numpy(c["w"].copy())[:, :, None].requires_grad_()
    b = torch.from_numpy(c["bias"].copy()).requires_grad_() if c["bias"] is not None else None
    y = F.conv1d(x, w, b)
    y.backward(torch.from_numpy(c["g"].copy()))
    out = dict(y=y.detach().numpy(), dx=x.grad.numpy(), dw=w.grad.numpy()[:, :, 0])
    if b is not None:
        out["db"] = b.grad.numpy()
    return out


def test_bars_are_recomputed(one_thread):
    """BARS == pow2_at_or_above(4 x REF_UNITS), exactly.  What is measured again here -- torch's CPU float32 ``F.conv1d`` and its
    autograd against the float64 oracle, worst over the matrix -- is held to REF_UNITS within a factor of 2, not to equality:
    torch's CPU convolution takes other code paths on other processors (tests/test_linear_wgrad_ref.py).  The bars the device is
    held to are the table's."""
    for q in pm.QUANTITIES:
        assert pm.BARS[q] == pow2_at_or_above(4 * pm.REF_UNITS[q]), (q, pm.BARS[q], pm.REF_UNITS[q])
    worst = {q: (0.0, "") for q in pm.QUANTITIES}
    for name in pm.case_names():
        u, bad = pm.units(name, _torch_run(pm.load_case(name)))
        assert not bad, (name, bad)
        for q, v in u.items():
            if v > worst[q][0]:
                worst[q] = (v, name)
    for q in pm.QUANTITIES:
        print(f"{q}: torch's worst units {worst[q][0]:.2f} ({worst[q][1]}) -> bar {pow2_at_or_above(4 * worst[q][0])}")
    for q in pm.QUANTITIES:
        assert 0.5 * pm.REF_UNITS[q] <= worst[q][0] <= 2.0 * pm.REF_UNITS[q], (q, worst[q], pm.REF_UNITS[q])


@pytest.mark.parametrize("name", pm.small_case_names())
def test_emulation_is_under_the_bars(name):
    """The arithmetic of csrc/pointwise_conv_plan.h, in numpy, on every case but the recipes': classes exactly, under the bars,
    and inside the element bounds."""
    got = pm.emulated(name)
    u, bad = pm.units(name, got)
    excess = pm.element_excess(name, got)
    print(f"{name}: emulation " + " ".join(f"{q} {u[q]:.2f} ({excess[q]:.3f})" for q in pm.QUANTITIES) + "  units (element bound used)")
    assert not bad, (name, bad)
    for q in pm.QUANTITIES:
        assert u[q] <= pm.BARS[q], (name, q, u[q])
        assert excess[q] <= 1.0, (name, q, excess[q])


def test_emulation_is_the_linear_contract_on_the_transposes():
    """dw and db of the emulation are tests/linear_wgrad_ref.emulate on x.transpose(1, 2).reshape(R, Ci) and the like, under the
    plan wekws_hip_linear_wgrad_plan(B T, Co, Ci) reports; a forward without a bias is never -0."""
    c, s = pm.load_case("chain600"), pm.cases()["chain600"]
    xt = torch.from_numpy(c["x"].copy()).transpose(1, 2).reshape(-1, s["Ci"]).numpy()
    gt = torch.from_numpy(c["g"].copy()).transpose(1, 2).reshape(-1, s["Co"]).numpy()
    dw, db = pr.lr.emulate(xt, gt, lm.device_plan(s["B"] * s["T"], s["Co"], s["Ci"]))
    e = pm.emulated("chain600")
    assert np.array_equal(dw.view(np.uint32), e["dw"].view(np.uint32)) and np.array_equal(db.view(np.uint32), e["db"].view(np.uint32))
    x = np.array([[[1.0, -1.0, 0.0]]], np.float32)
    y = pr.emulate_forward(x, np.array([[-0.0]], np.float32))
    assert not np.signbit(y).any()


def test_nan_and_inf_cases_are_what_they_say():
    nan, inf = pm.oracle("nan"), pm.oracle("inf")
    hit = np.zeros(nan["y"].shape, bool)
    hit[pm.NAN_B, :, pm.NAN_T] = True
    assert np.isnan(nan["y"][hit]).all() and np.isfinite(nan["y"][~hit]).all() and np.isfinite(nan["dx"]).all()
    cols = [i for i in range(nan["dw"].shape[1]) if i != pm.NAN_I]
    assert np.isnan(nan["dw"][:, pm.NAN_I]).all() and np.isfinite(nan["dw"][:, cols]).all() and np.isfinite(nan["db"]).all()
    assert np.isinf(inf["dx"][pm.INF_B, :, pm.INF_T]).all() and np.isinf(inf["dw"][pm.INF_O]).all() and inf["db"][pm.INF_O] == np.inf
    e = pm.emulated("nan")
    assert np.isnan(e["y"][hit]).all() and np.isfinite(e["y"][~hit]).all()
    assert np.isnan(e["dw"][:, pm.NAN_I]).all() and np.isfinite(e["dw"][:, cols]).all()


def test_negative_control_misses_the_y_bar_by_far():
    """w rounded to float16 at ds_tcn, through the oracle itself: what reduced-precision products would cost."""
    c = pm.load_case(pm.CONTROL_CASE)
    w16 = c["w"].astype(np.float16).astype(np.float32)
    u = pm.tensor_units(pr.oracle(c["x"], w16, c["bias"], c["g"])["y"], pm.oracle(pm.CONTROL_CASE)["y"])
    print(f"negative control: y is {u:.0f} units from the oracle, bar {pm.BARS['y']}")
    assert u >= 8 * pm.BARS["y"] and abs(u - pm.CONTROL_UNITS) <= 0.01 * pm.CONTROL_UNITS


def test_plan_is_the_linear_weight_gradients_without_a_device():
    K = pm.chain_rows()
    assert K == lm.chain_rows()
    shapes = [(1, 1, 1, 1), (2, 16, 256, 16), (3, 8, 200, 8), (7, 2049, 1171, 2), (256, 64, 100, 64), (100, 80, 200, 32),
              (256, 256, 100, 256), (3, 65535, 5, 65535), (2 ** 20, 8, 2 ** 13, 8), (1, 4, 2 ** 31 - 1, 4), (2 ** 31 - 1, 4, 1, 4)]
    lib = _capi.load()
    for B, Ci, T, Co in shapes:
        rc, out = _plan(B, Ci, T, Co)
        assert rc == 0, (B, Ci, T, Co, _capi.last_error())
        lin = (ctypes.c_int64 * 5)()
        assert lib.wekws_hip_linear_wgrad_plan(B * T, Co, Ci, lin) == 0
        assert out[:5] == list(lin), (B, Ci, T, Co)
        tiles_t = -(-T // 64)
        assert out[5] == B * tiles_t * -(-Co // 64) and out[6] == B * tiles_t * -(-Ci // 64)
        assert lib.wekws_hip_pointwise_conv1d_workspace_bytes(B, Ci, T, Co) == out[4]
        assert out[4] == lib.wekws_hip_linear_wgrad_workspace_bytes(B * T, Co, Ci)


def test_plan_and_workspace_refusals_without_a_device():
    lib = _capi.load()
    for bad in ((0, 16, 5, 16), (-1, 16, 5, 16), (2, 0, 5, 16), (2, 16, 0, 16), (2, 16, -4, 16), (2, 16, 5, 0), (2, 65536, 5, 16),
                (2, 16, 5, 65536), (2, -3, 5, 16)):
        rc, _ = _plan(*bad)
        assert rc == -1 and "pointwise_conv1d_plan" in _capi.last_error(), bad             # WEKWS_HIP_EINVAL
        assert lib.wekws_hip_pointwise_conv1d_workspace_bytes(*bad) == 0, bad
        assert "pointwise_conv1d_workspace_bytes" in _capi.last_error()
    assert lib.wekws_hip_pointwise_conv1d_plan(2, 16, 5, 16, None) == -1
    # a grid beyond 2^31 - 1: 2^31 - 1 batch rows of two frame tiles
    rc, _ = _plan(2 ** 31 - 1, 4, 65, 4)
    assert rc == -1 and "grid" in _capi.last_error()


def test_call_refusals_before_any_launch():
    """Everything the two calls refuse, refused on the arguments alone: no device is touched, so host addresses serve."""
    lib = _capi.load()
    B, Ci, T, Co = 2, 16, 5, 12
    ws_bytes = lib.wekws_hip_pointwise_conv1d_workspace_bytes(B, Ci, T, Co)
    buf = (ctypes.c_char * (ws_bytes + 64))()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = base                                                           # any non-NULL operand address: never read
    forward = {
        "B < 1": (p, 0, Ci, T, p, p, Co, p),
        "Ci = 0": (p, B, 0, T, p, p, Co, p),
        "Ci too large": (p, B, 65536, T, p, p, Co, p),
        "T < 1": (p, B, Ci, 0, p, p, Co, p),
        "Co = 0": (p, B, Ci, T, p, p, 0, p),
        "Co too large": (p, B, Ci, T, p, p, 65536, p),
        "grid": (p, 2 ** 31 - 1, Ci, 65, p, p, Co, p),
        "x NULL": (None, B, Ci, T, p, p, Co, p),
        "w NULL": (p, B, Ci, T, None, p, Co, p),
        "y NULL": (p, B, Ci, T, p, p, Co, None),
    }
    for what, args in forward.items():
        assert lib.wekws_hip_pointwise_conv1d_forward(*args, None) == -1, what
        assert "pointwise_conv1d_forward" in _capi.last_error(), what
    backward = {
        "B < 1": (p, p, 0, Ci, T, p, Co, p, p, p, base, ws_bytes),
        "Ci = 0": (p, p, B, 0, T, p, Co, p, p, p, base, ws_bytes),
        "Ci too large": (p, p, B, 65536, T, p, Co, p, p, p, base, 2 ** 40),
        "T < 1": (p, p, B, Ci, 0, p, Co, p, p, p, base, ws_bytes),
        "Co = 0": (p, p, B, Ci, T, p, 0, p, p, p, base, ws_bytes),
        "Co too large": (p, p, B, Ci, T, p, 65536, p, p, p, base, 2 ** 40),
        "grid": (p, p, 2 ** 31 - 1, Ci, 65, p, Co, p, p, p, base, 2 ** 60),
        "no output": (p, p, B, Ci, T, p, Co, None, None, None, base, ws_bytes),
        "x NULL": (None, p, B, Ci, T, p, Co, p, p, p, base, ws_bytes),
        "grad_y NULL": (p, None, B, Ci, T, p, Co, p, p, p, base, ws_bytes),
        "w NULL": (p, p, B, Ci, T, None, Co, p, p, p, base, ws_bytes),
        "workspace NULL": (p, p, B, Ci, T, p, Co, p, p, p, None, ws_bytes),
        "workspace NULL, grad_bias alone": (p, p, B, Ci, T, p, Co, None, None, p, None, 0),
        "workspace unaligned": (p, p, B, Ci, T, p, Co, p, p, None, base + 8, ws_bytes),
        "workspace small": (p, p, B, Ci, T, p, Co, None, p, p, base, ws_bytes - 16),
    }
    for what, args in backward.items():
        assert lib.wekws_hip_pointwise_conv1d_backward(*args, None) == -1, what
        assert "pointwise_conv1d_backward" in _capi.last_error(), what


def test_raw_op_has_no_cpu_fallback():
    from wekws_amd.model import pointwise as pw
    with pytest.raises(ValueError, match="no CPU fallback"):
        pw.pointwise_conv1d(torch.zeros(2, 3, 4), torch.zeros(5, 3, 1))
