"""CPU: the bars of tests/linear_wgrad_matrix.py recomputed, the emulation of the kernel's arithmetic under them (the evidence
that they can be met before any GPU run), the negative control, and the plan of csrc/linear_wgrad_plan.h through the C ABI,
without a device: chain boundaries, slices, the workspace, monotonicity and every refusal."""
import ctypes

import numpy as np
import pytest
import torch

from tests import linear_wgrad_matrix as lm
from tests import linear_wgrad_ref as lr
from tests.helpers import pow2_at_or_above
from wekws_amd import _capi


@pytest.fixture(scope="module")
def one_thread():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                      # the sums' order, and so the recorded units, must not depend on the core count
    yield
    torch.set_num_threads(threads)


def _plan(R, O, I):
    out = (ctypes.c_int64 * 5)()
    rc = _capi.load().wekws_hip_linear_wgrad_plan(R, O, I, out)
    return rc, list(out)


def test_matrix_covers_what_it_says():
    K = lm.chain_rows()
    cases = lm.cases()
    assert {s["R"] for s in cases.values() if (s["O"], s["I"]) == (16, 16)} >= {1, 31, 32, 33, K - 1, K, K + 1, 2 * K + 1}
    edge = {1, 15, 16, 17, 63, 64, 65}
    assert {s["O"] for s in cases.values()} >= edge and {s["I"] for s in cases.values()} >= edge
    assert cases["odd"] == dict(R=1000, O=130, I=67, flavour="", bias=True, weight=True)
    s = cases["slices"]
    p = lm.device_plan(s["R"], s["O"], s["I"])
    assert p["slices"] >= 3 and p["chains_per_slice"] >= 2 and s["R"] % K != 0                     # a ragged last slice
    assert p["chains"] - (p["slices"] - 1) * p["chains_per_slice"] < p["chains_per_slice"]
    assert not cases["nobias"]["bias"] and not cases["now"]["weight"]
    assert {s["flavour"] for s in cases.values()} >= {"unaligned", "nan", "inf", "large", "recipe"}
    assert {(s["R"], s["O"], s["I"]) for s in cases.values() if s["flavour"] == "recipe"} == {
        (25600, 384, 128), (25600, 140, 400), (25600, 128, 250), (4096, 2599, 140)}
    large = lm.load_case("large")
    assert np.isfinite(lm.oracle("large")["dw"]).all() and np.abs(lm.oracle("large")["abs_dw"]).max() < 2.0 ** 127
    assert np.abs(large["x"]).max() > 2.0 ** 40


def test_bars_are_recomputed(one_thread):
    """BARS == pow2_at_or_above(4 x REF_UNITS), exactly.  What is measured again here -- torch's CPU float32 ``g.t().mm(x)`` and
    ``g.sum(0)`` against the float64 oracle, worst over the matrix -- is held to REF_UNITS within a factor of 2, not to equality:
    torch's CPU GEMM takes other code paths on other processors (tests/test_gru_train_ref.py).  The bars the device is held to
    are the table's."""
    for q in lm.QUANTITIES:
        assert lm.BARS[q] == pow2_at_or_above(4 * lm.REF_UNITS[q]), (q, lm.BARS[q], lm.REF_UNITS[q])
    worst = {q: (0.0, "") for q in lm.QUANTITIES}
    for name in lm.case_names():
        c = lm.load_case(name)
        x, g = torch.from_numpy(c["x"].copy()), torch.from_numpy(c["g"].copy())
        u, bad = lm.units(name, dict(dw=g.t().mm(x).numpy(), db=g.sum(0).numpy()))
        assert not bad, (name, bad)
        for q, v in u.items():
            if v > worst[q][0]:
                worst[q] = (v, name)
    for q in lm.QUANTITIES:
        print(f"{q}: torch's worst units {worst[q][0]:.2f} ({worst[q][1]}) -> bar {pow2_at_or_above(4 * worst[q][0])}")
    for q in lm.QUANTITIES:
        assert 0.5 * lm.REF_UNITS[q] <= worst[q][0] <= 2.0 * lm.REF_UNITS[q], (q, worst[q], lm.REF_UNITS[q])


@pytest.mark.parametrize("name", lm.small_case_names())
def test_emulation_is_under_the_bars(name):
    """The arithmetic of csrc/linear_wgrad_plan.h, in numpy, on every case but the recipes' (whose emulation would take minutes):
    classes exactly, under the bars, and inside the element bound."""
    got = lm.emulated(name)
    u, bad = lm.units(name, got)
    excess = lm.element_excess(name, got)
    print(f"{name}: emulation dw {u['dw']:.2f} db {u['db']:.2f} units; element bound used {excess['dw']:.3f} {excess['db']:.3f}")
    assert not bad, (name, bad)
    for q in lm.QUANTITIES:
        assert u[q] <= lm.BARS[q], (name, q, u[q])
        assert excess[q] <= 1.0, (name, q, excess[q])


def test_nan_and_inf_cases_are_what_they_say():
    nan, inf = lm.oracle("nan"), lm.oracle("inf")
    cols = [i for i in range(nan["dw"].shape[1]) if i != lm.NAN_I]
    assert np.isnan(nan["dw"][:, lm.NAN_I]).all() and np.isfinite(nan["dw"][:, cols]).all() and np.isfinite(nan["db"]).all()
    rows = [o for o in range(inf["dw"].shape[0]) if o != lm.INF_O]
    assert np.isinf(inf["dw"][lm.INF_O]).all() and np.isfinite(inf["dw"][rows]).all() and inf["db"][lm.INF_O] == np.inf
    e = lm.emulated("nan")
    assert np.isnan(e["dw"][:, lm.NAN_I]).all() and np.isfinite(e["dw"][:, cols]).all()


def test_fmaf32_is_a_correctly_rounded_fma():
    """Against exact rational arithmetic, on random values and on a sum that a plain double addition would round twice:
    (1 + 2^-23) + 2^-24 (1 - 2^-46) is below the float32 tie, but its double rounding is the tie itself."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(200).astype(np.float32), rng.standard_normal(200).astype(np.float32)
    c = (rng.standard_normal(200) * 2.0 ** rng.integers(-30, 30, 200)).astype(np.float32)
    a[0], b[0], c[0] = np.float32(2.0 ** -12 * (1 + 2.0 ** -23)), np.float32(2.0 ** -12 * (1 - 2.0 ** -23)), np.float32(1 + 2.0 ** -23)
    got = lr.fmaf32(a, b, c)
    assert got[0] == np.float32(1 + 2.0 ** -23)
    assert np.float32(float(a[0]) * float(b[0]) + float(c[0])) == np.float32(1 + 2.0 ** -22)       # the double rounding it avoids
    for k in range(200):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        near = np.float32(float(exact))
        cands = [np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.int32)) & 1))
        assert got[k] == best, (k, got[k], best)


def test_negative_control_misses_the_dw_bar_by_far():
    """x rounded to float16 at gru_ih, through the oracle itself: what reduced-precision products would cost."""
    c = lm.load_case("gru_ih")
    x16 = c["x"].astype(np.float16).astype(np.float32)
    u = lm.tensor_units(lr.oracle(x16, c["g"])["dw"], lm.oracle("gru_ih")["dw"])
    print(f"negative control: dw is {u:.0f} units from the oracle, bar {lm.BARS['dw']}")
    assert u >= 8 * lm.BARS["dw"] and abs(u - lm.CONTROL_UNITS) <= 0.01 * lm.CONTROL_UNITS


def test_plan_chains_slices_and_workspace_without_a_device():
    K = lm.chain_rows()
    assert K >= 32 and K % 32 == 0
    shapes = [(1, 1, 1), (K, 16, 16), (K + 1, 16, 16), (2 * K + 1, 16, 16), (1000, 130, 67), (25600, 384, 128), (25600, 140, 400),
              (25600, 128, 250), (4096, 2599, 140), (16 * K + 5, 2, 2049), (10 ** 7, 64, 64), (3, 65535, 65535), (2 ** 33, 8, 8)]
    lib = _capi.load()
    for R, O, I in shapes:
        rc, (chain, chains, slices, grid, ws) = _plan(R, O, I)
        assert rc == 0, (R, O, I)
        pad = lambda n: -(-n // 64) * 64  # noqa: E731
        tiles = (pad(O) // 64) * (pad(I) // 64)
        assert chain == K and chains == -(-R // K)                       # chain c is rows [c K, min(R, (c + 1) K)), whatever O and I
        assert 1 <= slices <= chains and grid == tiles * slices
        assert slices == chains or tiles * slices <= 512                 # about 512 workgroups, never fewer chains than slices
        cps = -(-chains // slices)
        assert (slices - 1) * cps < chains <= slices * cps               # runs of cps consecutive chains, the last one shorter
        doubles = slices * pad(O) * pad(I) + slices * pad(O)
        assert ws == -(-doubles * 8 // 16) * 16
        assert lib.wekws_hip_linear_wgrad_workspace_bytes(R, O, I) == ws
    # the chain boundaries do not depend on O or I; slices and the workspace never shrink as R grows
    for O, I in ((16, 16), (384, 128), (2599, 140)):
        last = (0, 0, 0)
        for R in list(range(1, 4 * K + 2, 37)) + [25600, 10 ** 6]:
            rc, (chain, chains, slices, grid, ws) = _plan(R, O, I)
            assert rc == 0 and chains == -(-R // K) and chains >= last[0] and ws >= last[2], (R, O, I)
            last = (chains, slices, ws)


def test_plan_and_workspace_refusals_without_a_device():
    lib = _capi.load()
    for bad in ((0, 16, 16), (-1, 16, 16), (5, 0, 16), (5, 16, 0), (5, 65536, 16), (5, 16, 65536), (5, -3, 16)):
        rc, _ = _plan(*bad)
        assert rc == -1 and "linear_wgrad_plan" in _capi.last_error(), bad             # WEKWS_HIP_EINVAL
        assert lib.wekws_hip_linear_wgrad_workspace_bytes(*bad) == 0, bad
        assert "linear_wgrad_workspace_bytes" in _capi.last_error()
    assert lib.wekws_hip_linear_wgrad_plan(5, 16, 16, None) == -1


def test_call_refusals_before_any_launch():
    """Everything wekws_hip_linear_wgrad refuses, refused on the arguments alone: no device is touched, so host addresses serve."""
    lib = _capi.load()
    ws_bytes = lib.wekws_hip_linear_wgrad_workspace_bytes(5, 16, 16)
    buf = (ctypes.c_char * (ws_bytes + 64))()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = base                                                           # any non-NULL operand address: never read
    calls = {
        "R < 1": (p, p, 0, 16, 16, p, p, base, ws_bytes),
        "O = 0": (p, p, 5, 0, 16, p, p, base, ws_bytes),
        "O too large": (p, p, 5, 65536, 16, p, p, base, 2 ** 40),
        "I = 0": (p, p, 5, 16, 0, p, p, base, ws_bytes),
        "I too large": (p, p, 5, 16, 65536, p, p, base, 2 ** 40),
        "no output": (p, p, 5, 16, 16, None, None, base, ws_bytes),
        "x NULL": (None, p, 5, 16, 16, p, p, base, ws_bytes),
        "g NULL": (p, None, 5, 16, 16, p, p, base, ws_bytes),
        "workspace NULL": (p, p, 5, 16, 16, p, p, None, ws_bytes),
        "workspace unaligned": (p, p, 5, 16, 16, p, p, base + 8, ws_bytes),
        "workspace small": (p, p, 5, 16, 16, p, p, base, ws_bytes - 16),
    }
    for what, args in calls.items():
        assert lib.wekws_hip_linear_wgrad(*args, None) == -1, what
        assert "linear_wgrad" in _capi.last_error(), what


def test_raw_op_has_no_cpu_fallback():
    from wekws_amd.model import linear as dl
    with pytest.raises(ValueError):
        dl.linear_weight_grad(torch.zeros(4, 3), torch.zeros(4, 2))
    with pytest.raises(ValueError):
        dl.linear(torch.zeros(4, 3), torch.zeros(2, 3))
