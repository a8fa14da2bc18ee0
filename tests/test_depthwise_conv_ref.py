"""CPU: the float64 oracle of the depthwise Conv1d against the live reference's goldens, torch's CPU convolution against the
golden y bit for bit, the bars of tests/depthwise_conv_matrix.py recomputed, and the C entry points' plan and refusals (no
device needed)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import depthwise_conv_matrix as dm
from tests import depthwise_conv_ref as dr
from tests.helpers import pow2_at_or_above
from wekws_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "depthwise_conv_golden.npz"))


def torch_path(name, dtype=torch.float32):
    """torch's own statement on the CPU, ``F.conv1d(F.pad(x, (P, 0)), w, bias, dilation=d, groups=C)``: dict(y[, dx, dw, db])."""
    c = dm.load_case(name)
    C, K = c["w"].shape
    x = torch.from_numpy(c["x"].copy()).to(dtype).requires_grad_()
    w = torch.from_numpy(c["w"].copy()).to(dtype).view(C, 1, K).requires_grad_()
    b = torch.from_numpy(c["bias"].copy()).to(dtype).requires_grad_() if c["bias"] is not None else None
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                      # the sums' order, and so the recorded units, must not depend on the core count
    try:
        y = F.conv1d(F.pad(x, (c["P"], 0), value=0.0), w, b, dilation=c["d"], groups=C)
        out = {"y": y.detach().numpy()}
        if c["backward"]:
            y.backward(torch.from_numpy(c["g"].copy()).to(dtype))
            out.update(dx=x.grad.numpy(), dw=w.grad.numpy().reshape(C, K))
            if b is not None:
                out["db"] = b.grad.numpy()
    finally:
        torch.set_num_threads(threads)
    return out


def test_matrix_covers_what_it_says():
    names = dm.case_names()
    assert len(names) == len(set(names)) and set(dm.GOLDEN) <= set(names)
    shapes = [dm.CASES[n] for n in names]
    R, FT, GT = dr.ROWS, dr.FIR_TILE, dr.GRAD_TILE
    assert {s[0] * s[1] for s in shapes} >= {1, 3, 4, 5, R - 1, R, R + 1, 64, 66}
    assert {s[0] for s in shapes} >= {1, 2, 3, 4, 5}
    assert {(s[3], s[4]) for s in shapes} >= set(dm.TAP_SETS.values()) | {(32, 8)}
    assert {s[6] for s in shapes} == {True, False}
    tout = lambda s: dr.tout(s[2], s[3], s[4], s[5])  # noqa: E731
    for K, d in dm.TAP_SETS.values():
        w = dr.window(K, d)
        assert {tout(s) for s in shapes if (s[3], s[4]) == (K, d)} >= {t for t in (1, 2, w - 1, w, w + 1) if t >= 1}
    assert {tout(s) for s in shapes if (s[3], s[4]) == (8, 8)} >= {FT - 1, FT, FT + 1, 2 * FT + 3, GT - 1, GT, GT + 1, 2 * GT + 3}
    for K, d in ((8, 8), (5, 4)):
        assert {s[5] for s in shapes if (s[3], s[4]) == (K, d)} >= {0, 1, (K - 1) * d - 1, (K - 1) * d}
    assert {(s[2] % 4, tout(s) % 4) for s in shapes} == {(a, b) for a in range(4) for b in range(4)}
    assert any(tout(s) < dr.window(s[3], s[4]) and s[2] < dr.window(s[3], s[4]) and s[5] > 0 for s in shapes)
    n = {dr.partials(s[0], tout(s)) for s in shapes}
    assert any(v <= dr.FOLD_SEGS for v in n) and any(v > dr.FOLD_SEGS and v % dr.fold_seg_len(v) == 1 for v in n)
    assert any(v > dr.FOLD_SEGS and v % dr.fold_seg_len(v) > 1 for v in n)
    assert dm.CASES["recipe_tcn"][:6] == (256, 64, 100, 8, 8, 56) and dm.CASES["recipe_mdtc"][:6] == (100, 32, 200, 5, 8, 32)
    assert dr.window(*dm.CASES["long"][3:5]) == 249
    for name in names:
        assert dr.check(*dm.CASES[name][:6]), name


@pytest.mark.parametrize("name", sorted(dm.GOLDEN))
def test_oracle_equals_the_reference_in_float64(golden, name):
    c = dm.load_case(name)
    for k in ("x", "g", "w", "bias"):
        if c[k] is not None:
            assert np.array_equal(golden[f"{name}/{k}"], c[k], equal_nan=True)       # the golden was made from these inputs
        else:
            assert f"{name}/{k}" not in golden
    ref, mag = dm.oracle(name)
    assert c["bias"] is None or not c["backward"] or f"{name}/db64" in golden
    for k in ref:
        if f"{name}/{k}64" not in golden:
            assert k == "db" and c["bias"] is None
            continue
        want = golden[f"{name}/{k}64"]
        assert dm.same_classes(ref[k], want), (name, k)
        fin = np.isfinite(want)
        dev = np.abs(ref[k][fin] - want[fin])
        assert np.all(dev <= 1e-12 * mag[k][fin]), (name, k, float(dev.max()))


@pytest.mark.parametrize("name", sorted(dm.GOLDEN))
def test_torch_path_equals_the_reference_bit_for_bit(golden, name):
    got = torch_path(name)
    assert np.array_equal(got["y"].view(np.int32), golden[f"{name}/y32"].view(np.int32)), name
    u, bad = dm.units(name, {k: golden[f"{name}/{k}32"] for k in got})
    assert not bad and all(u[k] <= dm.BARS[k] for k in u), (name, u, bad)         # the live reference is within its own bars


def test_bars_are_recomputed():
    worst = {k: (0.0, "") for k in dm.QUANTITIES}
    for name in dm.case_names():
        got = torch_path(name)
        u, bad = dm.units(name, got)
        assert not bad, (name, bad)
        for k, v in u.items():
            if v > worst[k][0]:
                worst[k] = (v, name)
    for k in dm.QUANTITIES:
        print(f"{k}: reference's worst units {worst[k][0]:.2f} ({worst[k][1]}) -> bar {pow2_at_or_above(4 * worst[k][0])}")
    for k in dm.QUANTITIES:
        assert abs(worst[k][0] - dm.REF_UNITS[k]) < 0.01, (k, worst[k], dm.REF_UNITS[k])
        assert dm.BARS[k] == pow2_at_or_above(4 * worst[k][0]), (k, worst[k], dm.BARS[k])


def test_left_pad_is_the_padding_of_the_input():
    """The oracle's left_pad against itself on an explicitly padded x, and the padding's arithmetic zeros under an Inf tap."""
    c = dm.load_case("p55_k8d8")
    y, _ = dr.forward(c["x"], c["w"], c["bias"], c["d"], c["P"])
    xp = np.concatenate([np.zeros(c["x"].shape[:2] + (c["P"],), np.float32), c["x"]], axis=2)
    y0, _ = dr.forward(xp, c["w"], c["bias"], c["d"], 0)
    assert np.array_equal(y, y0)
    r, _ = dr.backward(c["x"], c["g"], c["w"], c["d"], c["P"])
    r0, _ = dr.backward(xp, c["g"], c["w"], c["d"], 0)
    assert np.array_equal(r["dx"], r0["dx"][:, :, c["P"]:]) and np.array_equal(r["dw"], r0["dw"]) and np.array_equal(r["db"], r0["db"])
    ref, _ = dm.oracle("g_inf_tap")
    P = dm.CASES["g_inf_tap"][5]
    assert np.isnan(ref["y"][:, 1, :P]).all() and np.isinf(ref["y"][:, 1, P:]).all() and np.isfinite(ref["y"][:, 0]).all()


def test_workspace_size_and_plan_without_a_device():
    lib = _capi.load()
    for name in dm.case_names():
        args = dm.CASES[name][:6]
        assert lib.wekws_hip_depthwise_conv1d_workspace_bytes(*args) == dr.workspace_bytes(*args), name
    assert dr.workspace_bytes(256, 64, 100, 8, 8, 56) == 256 * 64 * 9 * 8
    assert dr.workspace_bytes(100, 32, 200, 5, 8, 32) == 200 * 32 * 6 * 8
    assert dr.workspace_bytes(1, 1, 3, 2, 1, 0) % 16 == 0 and dr.workspace_bytes(1, 1, 3, 2, 1, 0) == 32
    # 64-bit sizes: 2^16 batch rows of two tiles, 4096 channels, 32 taps and the bias -> above 2^35 bytes
    assert lib.wekws_hip_depthwise_conv1d_workspace_bytes(1 << 16, 4096, 129, 32, 1, 31) == (1 << 17) * 4096 * 33 * 8
    for bad in ((0, 5, 9, 3, 1, 0), (2, 0, 9, 3, 1, 0), (2, 5, 0, 3, 1, 0), (-1, 5, 9, 3, 1, 0), (2, 5, 9, 0, 1, 0), (2, 5, 9, 33, 1, 0),
                (2, 5, 9, 3, 0, 0), (2, 5, 300, 32, 9, 0), (2, 5, 9, 3, 1, -1), (2, 5, 9, 3, 1, 3), (2, 5, 2, 3, 1, 0), (2, 5, 4, 3, 2, 0)):
        assert lib.wekws_hip_depthwise_conv1d_workspace_bytes(*bad) == 0 and _capi.last_error() != "", bad
        assert not dr.check(*bad), bad
    assert dr.taps(8, 8)[0] == (dr.LEFT, 0, 56) and dr.taps(8, 8)[7] == (dr.LEFT, 7, 0) and dr.window(8, 8) == 57
    assert dr.window(32, 8) == 249 and dr.check(1, 1, 249, 32, 8, 0) and not dr.check(1, 1, 300, 32, 9, 0)
    # the dynamic LDS of the longest window stays far below a workgroup's 64 KiB
    assert dr.fir_lds_bytes(256) == 8 * (388 + 128 + 33) * 4 and dr.grad_lds_bytes(256) == 8 * (388 + 128) * 4


def test_every_refusal_holds_without_a_device():
    """Argument errors return EINVAL with a message before any launch: nothing here needs (or touches) a device, so the
    pointers are host addresses that are never dereferenced."""
    lib = _capi.load()
    buf = np.zeros(4096, np.float64)
    p = buf.ctypes.data
    assert p % 16 == 0
    ws_bytes = dr.workspace_bytes(2, 5, 9, 3, 2, 4)

    def fwd(x=p, B=2, C=5, T=9, w=p, bias=p, K=3, d=2, P=4, y=p):
        return lib.wekws_hip_depthwise_conv1d_forward(x, B, C, T, w, bias, K, d, P, y, None)

    def bwd(x=p, g=p, B=2, C=5, T=9, w=p, K=3, d=2, P=4, dx=p, dw=p, db=p, ws=p, nb=ws_bytes):
        return lib.wekws_hip_depthwise_conv1d_backward(x, g, B, C, T, w, K, d, P, dx, dw, db, ws, nb, None)

    shape_errors = [dict(B=0), dict(C=0), dict(T=0), dict(B=-3), dict(K=0), dict(K=33), dict(d=0), dict(d=-1), dict(K=32, d=9, T=400, P=0),
                    dict(K=3, d=128, T=400, P=0), dict(P=-1), dict(P=5), dict(T=4, P=0), dict(T=1, P=3)]
    for call, nulls in ((fwd, ("x", "w", "y")), (bwd, ("x", "g", "w"))):
        for k in nulls:
            assert call(**{k: None}) == -1 and "NULL" in _capi.last_error(), k
        for kw in shape_errors:
            assert call(**kw) == -1 and _capi.last_error() != "", kw
    assert "K must" in (fwd(K=33), _capi.last_error())[1] and "window" in (fwd(K=3, d=128, T=400, P=0), _capi.last_error())[1]
    assert "left_pad" in (fwd(P=5), _capi.last_error())[1] and "no output frame" in (fwd(T=4, P=0), _capi.last_error())[1]
    # a window of exactly 256 frames is inside the limits: refused for nothing but the missing workspace here
    assert bwd(K=16, d=17, T=300, P=0, ws=None) == -1 and "workspace" in _capi.last_error()
    assert bwd(nb=ws_bytes - 1) == -1 and "workspace" in _capi.last_error()
    assert bwd(nb=0) == -1 and bwd(ws=None) == -1
    assert bwd(ws=p + 8) == -1 and "aligned" in _capi.last_error()
    assert bwd(dw=None, ws=None) == -1 and bwd(db=None, ws=None) == -1           # either gradient alone still needs the workspace
    assert not buf.any()
