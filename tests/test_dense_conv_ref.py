"""CPU: the oracle of tests/dense_conv_ref.py against the live reference's goldens, the bars of tests/dense_conv_matrix.py
recomputed, the emulation of the kernels' arithmetic under them and inside the element bounds (the evidence that they can be met
before any GPU run), the negative control, and the plan of csrc/dense_conv_plan.h through the C ABI, without a device: against
the Linear weight gradient's plan and the header's arithmetic, and every refusal."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dense_conv_matrix as dm
from tests import dense_conv_ref as dr
from tests import linear_wgrad_matrix as lm
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
    return np.load(os.path.join(ROOT, "tests", "golden", "dense_conv_golden.npz"))


def _plan(*shape):
    out = (ctypes.c_int64 * 10)()
    rc = _capi.load().wekws_hip_dense_conv1d_plan(*shape, out)
    return rc, list(out)


def test_matrix_covers_what_it_says():
    chain = dm.chain_rows()
    cases = dm.cases()
    edge = [s for s in cases.values() if (s["B"], s["Ci"], s["Co"], s["K"], s["d"], s["P"]) == (2, 16, 16, 3, 2, 4)]
    assert {s["Tout"] for s in edge} >= {1, 15, 16, 17, 63, 64, 65, 129}
    shifts = {k * s["d"] - s["P"] for s in cases.values() for k in range(s["K"])}
    assert all(any(v % 4 == r and v > 0 for v in shifts) and any(v % 4 == r and v < 0 for v in shifts) for r in range(4))
    assert {s["K"] for s in cases.values()} >= {1, 2, 3, 8} and {s["d"] for s in cases.values()} >= {1, 2, 3, 8}
    pads = [(s["P"], (s["K"] - 1) * s["d"]) for s in cases.values() if s["K"] > 1]
    assert any(p == 0 for p, _ in pads) and any(0 < p < full for p, full in pads) and any(p == full for p, full in pads)
    s = cases["subsampling"]
    assert (s["K"], s["d"], s["P"]) == (3, 1, 0) and s["Ci"] != s["Co"]
    s = cases["short"]
    assert (s["Tin"], s["K"], s["d"], s["P"]) == (3, 8, 1, 7)
    assert [(cases[n]["K"], cases[n]["d"]) for n in ("window_k2", "window_k32")] == [(2, 255), (32, 8)]
    assert all((cases[n]["K"] - 1) * cases[n]["d"] + 1 in (256, 249) for n in ("window_k2", "window_k32"))
    sweep = [s for s in cases.values() if (s["B"], s["Tin"], s["K"]) == (2, 35, 3)]
    want = {1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65}
    assert {s["Ci"] for s in sweep} >= want and {s["Co"] for s in sweep} >= want
    assert 2 * cases["chain600"]["Tout"] < chain < 3 * cases["chain600"]["Tout"]     # the chain boundary falls inside batch row 2
    assert cases["straddle"]["Tout"] % 32 != 0 and cases["straddle"]["Tout"] % 4 != 0
    assert [cases[n]["B"] * cases[n]["Tout"] for n in ("rK-1", "rK", "rK+1", "r2K+1")] == [chain - 1, chain, chain + 1, 2 * chain + 1]
    s = cases["slices"]
    p = dm.device_plan(s["B"], s["Ci"], s["Tin"], s["Co"], s["K"], s["d"], s["P"])
    assert p["slices"] >= 3 and p["chains_per_slice"] >= 2 and (s["B"] * s["Tout"]) % chain != 0          # a ragged last slice
    assert p["chains"] - (p["slices"] - 1) * p["chains_per_slice"] < p["chains_per_slice"]
    assert not cases["nobias"]["bias"] and "db" not in cases["nobias"]["wants"]
    assert [set(cases[n]["wants"]) for n in ("nodx", "nodw", "nodb")] == [{"dw", "db"}, {"dx", "db"}, {"dx", "dw"}]
    assert {s["flavour"] for s in cases.values()} >= {"unaligned", "nan", "inf", "winf", "large", "recipe"}
    assert cases["winf"]["wants"] == () and cases["winf"]["P"] > 0
    assert {(s["B"], s["Ci"], s["Co"], s["Tin"], s["K"], s["d"], s["P"]) for s in cases.values() if s["flavour"] == "recipe"} == {
        (256, 64, 64, 100, 8, d, 7 * d) for d in (1, 2, 4, 8)}
    o = dm.oracle("large")
    assert all(np.isfinite(o[q]).all() for q in dm.QUANTITIES) and max(np.abs(o["abs_" + q]).max() for q in dm.QUANTITIES) < 2.0 ** 127
    assert np.abs(dm.load_case("large")["x"]).max() > 2.0 ** 40
    assert set(dm.GOLDEN) <= set(dm.small_case_names()) and 5 <= len(dm.GOLDEN) <= 6


@pytest.mark.parametrize("name", sorted(dm.GOLDEN))
def test_oracle_against_the_references_golden(golden, name):
    """The seeded inputs are the recorded ones; the float64 oracle is the reference's float64 convolution behind its F.pad and
    autograd to a few units of 2^-53, and the reference's float32 run is inside the bars."""
    c, ref = dm.load_case(name), dm.oracle(name)
    for k in ("x", "g", "w", "bias"):
        assert np.array_equal(c[k], golden[f"{name}/{k}"]), (name, k)
    for q in dm.QUANTITIES:
        g64 = golden[f"{name}/{q}64"]
        assert g64.shape == ref[q].shape
        assert np.abs(g64 - ref[q]).max() <= 2.0 ** -40 * np.abs(ref[q]).max(), (name, q)
    u, bad = dm.units(name, {q: golden[f"{name}/{q}32"] for q in dm.QUANTITIES})
    assert not bad
    for q in dm.QUANTITIES:
        assert u[q] <= dm.BARS[q], (name, q, u[q])


def _torch_run(c):
    s = c["spec"]
    x = torch.from_numpy(c["x"].copy()).requires_grad_()
    w = torch.from_numpy(c["w"].copy()).requires_grad_()
    b = torch.from_numpy(c["bias"].copy()).requires_grad_() if c["bias"] is not None else None
    y = F.conv1d(F.pad(x, (s["P"], 0)), w, b, dilation=s["d"])
    out = dict(y=y.detach().numpy())
    if s["wants"]:
        y.backward(torch.from_numpy(c["g"].copy()))
        out.update(dx=x.grad.numpy(), dw=w.grad.numpy())
        if b is not None:
            out["db"] = b.grad.numpy()
    return out


def test_bars_are_recomputed(one_thread):
    """BARS == pow2_at_or_above(4 x REF_UNITS), exactly.  What is measured again here -- torch's CPU float32 ``F.conv1d`` behind
    ``F.pad`` and its autograd against the float64 oracle, worst over the matrix -- is held to REF_UNITS within a factor of 2, not
    to equality: torch's CPU convolution takes other code paths on other processors (tests/test_linear_wgrad_ref.py).  The bars
    the device is held to are the table's."""
    for q in dm.QUANTITIES:
        assert dm.BARS[q] == pow2_at_or_above(4 * dm.REF_UNITS[q]), (q, dm.BARS[q], dm.REF_UNITS[q])
    worst = {q: (0.0, "") for q in dm.QUANTITIES}
    for name in dm.case_names():
        u, bad = dm.units(name, _torch_run(dm.load_case(name)))
        assert not bad, (name, bad)
        for q, v in u.items():
            if v > worst[q][0]:
                worst[q] = (v, name)
    for q in dm.QUANTITIES:
        print(f"{q}: torch's worst units {worst[q][0]:.2f} ({worst[q][1]}) -> bar {pow2_at_or_above(4 * worst[q][0])}")
    for q in dm.QUANTITIES:
        assert 0.5 * dm.REF_UNITS[q] <= worst[q][0] <= 2.0 * dm.REF_UNITS[q], (q, worst[q], dm.REF_UNITS[q])


@pytest.mark.parametrize("name", dm.small_case_names())
def test_emulation_is_under_the_bars(name):
    """The arithmetic of csrc/dense_conv_plan.h, in numpy, on every case but the recipe's: classes exactly, under the bars, and
    inside the element bounds."""
    got = dm.emulated(name)
    u, bad = dm.units(name, got)
    excess = dm.element_excess(name, got)
    print(f"{name}: emulation " + " ".join(f"{q} {u[q]:.2f} ({excess[q]:.3f})" for q in got) + "  units (element bound used)")
    assert not bad, (name, bad)
    for q in got:
        assert u[q] <= dm.BARS[q], (name, q, u[q])
        assert excess[q] <= 1.0, (name, q, excess[q])


def test_emulation_is_the_linear_contract_on_the_shifted_transposes():
    """dw[:, :, k] and db of the emulation are tests/linear_wgrad_ref.emulate on the shifted, zero-padded, transposed copies under
    the plan wekws_hip_linear_wgrad_plan(B Tout, Co, Ci) reports, made here with torch's own pad and slice; with K = 1 the
    emulation is the pointwise one's; a forward without a bias is never -0."""
    from tests import pointwise_conv_ref as pr
    c, s = dm.load_case("chain600"), dm.cases()["chain600"]
    xp = F.pad(torch.from_numpy(c["x"].copy()), (s["P"], 0))
    gt = torch.from_numpy(c["g"].copy()).transpose(1, 2).reshape(-1, s["Co"]).numpy()
    e = dm.emulated("chain600")
    plan = lm.device_plan(s["B"] * s["Tout"], s["Co"], s["Ci"])
    for k in range(s["K"]):
        xt = xp[:, :, k * s["d"]:k * s["d"] + s["Tout"]].transpose(1, 2).reshape(-1, s["Ci"]).numpy()
        dw, db = dr.lr.emulate(xt, gt, plan)
        assert np.array_equal(dw.view(np.uint32), e["dw"][:, :, k].view(np.uint32)), k
        assert np.array_equal(db.view(np.uint32), e["db"].view(np.uint32))
    c, s, e = dm.load_case("k1"), dm.cases()["k1"], dm.emulated("k1")
    w2 = c["w"][:, :, 0]
    assert np.array_equal(e["y"].view(np.uint32), pr.emulate_forward(c["x"], w2, c["bias"]).view(np.uint32))
    assert np.array_equal(e["dx"].view(np.uint32), pr.emulate_dx(c["g"], w2).view(np.uint32))
    dw, db = pr.emulate_wgrad(c["x"], c["g"], lm.device_plan(s["B"] * s["Tout"], s["Co"], s["Ci"]))
    assert np.array_equal(e["dw"][:, :, 0].view(np.uint32), dw.view(np.uint32)) and np.array_equal(e["db"].view(np.uint32), db.view(np.uint32))
    x = np.array([[[1.0, -1.0, 0.0]]], np.float32)
    y = dr.emulate_forward(x, np.array([[[-0.0, -0.0]]], np.float32), None, 1, 1)
    assert y.shape == (1, 1, 3) and not np.signbit(y).any()


def test_nan_and_inf_cases_are_what_they_say():
    s = dm.cases()["nan"]
    frames, taps = dm.nan_hits(s)
    assert taps == [s["K"] - 1] and len(frames) == 1                       # the last tap alone reaches it
    nan, inf, winf = dm.oracle("nan"), dm.oracle("inf"), dm.oracle("winf")
    for ref in (nan, dm.emulated("nan")):
        hit = np.zeros(ref["y"].shape, bool)
        hit[dm.NAN_B, :, frames] = True
        assert np.isnan(ref["y"][hit]).all() and np.isfinite(ref["y"][~hit]).all() and np.isfinite(ref["dx"]).all()
        whit = np.zeros(ref["dw"].shape, bool)
        whit[:, dm.NAN_I, taps] = True
        assert np.isnan(ref["dw"][whit]).all() and np.isfinite(ref["dw"][~whit]).all() and np.isfinite(ref["db"]).all()
    assert np.isinf(inf["dw"][dm.INF_O]).any() and inf["db"][dm.INF_O] == np.inf and not np.isfinite(inf["dx"][dm.INF_B]).all()
    assert np.isfinite(inf["dx"][1 - dm.INF_B]).all()
    s = dm.cases()["winf"]
    for y in (winf["y"], dm.emulated("winf")["y"]):
        assert np.isnan(y[:, dm.WINF_O, :s["P"]]).all() and np.isinf(y[:, dm.WINF_O, s["P"]:]).all()
        assert np.isfinite(np.delete(y, dm.WINF_O, 1)).all()
    # the reference's statement itself
    c = dm.load_case("winf")
    t = F.conv1d(F.pad(torch.from_numpy(c["x"].copy()), (s["P"], 0)), torch.from_numpy(c["w"].copy()), torch.from_numpy(c["bias"].copy()),
                 dilation=s["d"]).numpy()
    assert dm.same_classes(t, winf["y"])


def test_negative_control_misses_the_y_bar_by_far():
    """w rounded to float16 at tcn_d4, through the oracle itself: what reduced-precision products would cost."""
    c, s = dm.load_case(dm.CONTROL_CASE), dm.cases()[dm.CONTROL_CASE]
    w16 = c["w"].astype(np.float16).astype(np.float32)
    u = dm.tensor_units(dr.oracle(c["x"], w16, c["bias"], c["g"], s["d"], s["P"])["y"], dm.oracle(dm.CONTROL_CASE)["y"])
    print(f"negative control: y is {u:.0f} units from the oracle, bar {dm.BARS['y']}")
    assert u >= 8 * dm.BARS["y"] and abs(u - dm.CONTROL_UNITS) <= 0.01 * dm.CONTROL_UNITS


SHAPES = [(1, 1, 1, 1, 1, 1, 0), (2, 16, 129, 16, 3, 2, 4), (3, 8, 200, 8, 3, 2, 4), (5, 1025, 3073, 2, 2, 1, 1), (256, 64, 100, 64, 8, 1, 7),
          (256, 64, 100, 64, 8, 8, 56), (2, 20, 50, 24, 3, 1, 0), (2, 16, 3, 16, 8, 1, 7), (2, 3, 40, 2, 2, 255, 255), (2, 2, 20, 3, 32, 8, 248),
          (3, 65535, 5, 65535, 2, 1, 1), (2 ** 20, 8, 2 ** 13, 8, 8, 4, 28), (1, 4, 2 ** 31 - 1, 4, 3, 1, 2), (2 ** 31 - 1, 4, 1, 4, 2, 1, 1),
          (2, 4, 256, 4, 32, 8, 0)]


def test_plan_is_the_linear_weight_gradients_and_the_headers_without_a_device():
    chain = dm.chain_rows()
    assert chain == lm.chain_rows()
    lib = _capi.load()
    for B, Ci, Tin, Co, K, d, P in SHAPES:
        rc, out = _plan(B, Ci, Tin, Co, K, d, P)
        assert rc == 0, (B, Ci, Tin, Co, K, d, P, _capi.last_error())
        Tout = Tin + P - (K - 1) * d
        lin = (ctypes.c_int64 * 5)()
        assert lib.wekws_hip_linear_wgrad_plan(B * Tout, Co, Ci, lin) == 0
        assert out[:4] == list(lin)[:4] and out[4] == K * lin[4], (B, Ci, Tin, Co, K, d, P)
        assert out[5] == B * -(-Tout // 64) * -(-Co // 64) and out[6] == B * -(-Tin // 64) * -(-Ci // 64)
        assert out[7] == K and out[8] == -(-(Co * Ci + Co) // 256) and out[9] == Tout
        assert lib.wekws_hip_dense_conv1d_workspace_bytes(B, Ci, Tin, Co, K, d, P) == out[4]
        assert out[4] == K * lib.wekws_hip_linear_wgrad_workspace_bytes(B * Tout, Co, Ci)


BAD_SHAPES = {
    "B = 0": (0, 16, 9, 16, 3, 1, 2), "B < 0": (-1, 16, 9, 16, 3, 1, 2), "Ci = 0": (2, 0, 9, 16, 3, 1, 2), "Ci < 0": (2, -3, 9, 16, 3, 1, 2),
    "Ci too large": (2, 65536, 9, 16, 3, 1, 2), "Tin = 0": (2, 16, 0, 16, 3, 1, 2), "Tin < 0": (2, 16, -4, 16, 3, 1, 2),
    "Co = 0": (2, 16, 9, 0, 3, 1, 2), "Co too large": (2, 16, 9, 65536, 3, 1, 2), "K = 0": (2, 16, 9, 16, 0, 1, 0),
    "K = 33": (2, 16, 64, 16, 33, 1, 32), "d = 0": (2, 16, 9, 16, 3, 0, 0), "window 257": (2, 16, 300, 16, 2, 256, 256),
    "window 257, K = 32": (2, 16, 300, 16, 33 - 1, 9, 0), "P < 0": (2, 16, 9, 16, 3, 1, -1), "P too large": (2, 16, 9, 16, 3, 1, 3),
    "no output frame": (2, 16, 2, 16, 3, 1, 0), "no output frame, padded": (2, 16, 3, 16, 8, 1, 4),
}


def test_plan_and_workspace_refusals_without_a_device():
    lib = _capi.load()
    for what, bad in BAD_SHAPES.items():
        rc, _ = _plan(*bad)
        assert rc == -1 and "dense_conv1d_plan" in _capi.last_error(), what             # WEKWS_HIP_EINVAL
        assert lib.wekws_hip_dense_conv1d_workspace_bytes(*bad) == 0, what
        assert "dense_conv1d_workspace_bytes" in _capi.last_error()
    assert lib.wekws_hip_dense_conv1d_plan(2, 16, 9, 16, 3, 1, 2, None) == -1
    # the limits' edges are accepted
    for ok in ((2, 16, 300, 16, 2, 255, 255), (2, 16, 300, 16, 32, 8, 248), (2, 16, 1, 16, 3, 1, 2), (2, 65535, 9, 65535, 3, 1, 2)):
        assert _plan(*ok)[0] == 0, ok
    # a grid beyond 2^31 - 1: 2^31 - 1 batch rows of two frame tiles
    rc, _ = _plan(2 ** 31 - 1, 4, 65, 4, 2, 1, 1)
    assert rc == -1 and "grid" in _capi.last_error()


def test_call_refusals_before_any_launch():
    """Everything the two calls refuse, refused on the arguments alone: no device is touched, so host addresses serve."""
    lib = _capi.load()
    B, Ci, Tin, Co, K, d, P = 2, 16, 9, 12, 3, 2, 4
    ws_bytes = lib.wekws_hip_dense_conv1d_workspace_bytes(B, Ci, Tin, Co, K, d, P)
    buf = (ctypes.c_char * (ws_bytes + 64))()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = base                                                           # any non-NULL operand address: never read
    forward = {what: (p, s[0], s[1], s[2], p, p, s[3], s[4], s[5], s[6], p) for what, s in BAD_SHAPES.items()}
    forward.update({
        "grid": (p, 2 ** 31 - 1, Ci, 65, p, p, Co, 2, 1, 1, p),
        "x NULL": (None, B, Ci, Tin, p, p, Co, K, d, P, p),
        "w NULL": (p, B, Ci, Tin, None, p, Co, K, d, P, p),
        "y NULL": (p, B, Ci, Tin, p, p, Co, K, d, P, None),
    })
    for what, args in forward.items():
        assert lib.wekws_hip_dense_conv1d_forward(*args, None) == -1, what
        assert "dense_conv1d_forward" in _capi.last_error(), what
    backward = {what: (p, p, s[0], s[1], s[2], p, s[3], s[4], s[5], s[6], p, p, p, base, 2 ** 40) for what, s in BAD_SHAPES.items()}
    backward.update({
        "grid": (p, p, 2 ** 31 - 1, Ci, 65, p, Co, 2, 1, 1, p, p, p, base, 2 ** 60),
        "no output": (p, p, B, Ci, Tin, p, Co, K, d, P, None, None, None, base, ws_bytes),
        "x NULL": (None, p, B, Ci, Tin, p, Co, K, d, P, p, p, p, base, ws_bytes),
        "grad_y NULL": (p, None, B, Ci, Tin, p, Co, K, d, P, p, p, p, base, ws_bytes),
        "w NULL": (p, p, B, Ci, Tin, None, Co, K, d, P, p, p, p, base, ws_bytes),
        "workspace NULL": (p, p, B, Ci, Tin, p, Co, K, d, P, p, p, p, None, ws_bytes),
        "workspace NULL, grad_bias alone": (p, p, B, Ci, Tin, p, Co, K, d, P, None, None, p, None, 0),
        "workspace unaligned": (p, p, B, Ci, Tin, p, Co, K, d, P, p, p, None, base + 8, ws_bytes),
        "workspace small": (p, p, B, Ci, Tin, p, Co, K, d, P, None, p, p, base, ws_bytes - 16),
        "workspace of one tap": (p, p, B, Ci, Tin, p, Co, K, d, P, None, p, p, base, ws_bytes // K),
    })
    for what, args in backward.items():
        assert lib.wekws_hip_dense_conv1d_backward(*args, None) == -1, what
        assert "dense_conv1d_backward" in _capi.last_error(), what


def test_raw_op_refusals_and_no_cpu_fallback():
    from wekws_amd.model import dense
    with pytest.raises(ValueError, match="no CPU fallback"):
        dense.dense_conv1d(torch.zeros(2, 3, 8), torch.zeros(5, 3, 2))
    assert dense.in_device_limits(32, 8) and dense.in_device_limits(2, 255) and not dense.in_device_limits(2, 256)
    assert not dense.in_device_limits(33, 1) and not dense.in_device_limits(3, 0) and not dense.in_device_limits("a", 1)
