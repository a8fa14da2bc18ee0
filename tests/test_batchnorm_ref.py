"""CPU: the float64 oracle of the BatchNorm1d sites against the live reference's goldens, torch's CPU float32 path within the bars
of tests/batchnorm_matrix.py, the bars recomputed, and the C entry points' plan and refusals (no device needed)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import batchnorm_matrix as bm
from tests import batchnorm_ref as br
from tests.helpers import pow2_at_or_above
from wekws_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "batchnorm_golden.npz"))


def torch_path(name, dtype=torch.float32):
    """torch's own statements on the CPU, ``relu(F.batch_norm(...) + residual)`` and their autograd, over the case's calls: a
    dict over the case's quantities (mean and invstd from ``x.mean`` / ``x.var``: torch keeps its saved statistics to itself)."""
    c = bm.load_case(name)
    t = lambda a, grad=False: torch.from_numpy(a.copy()).to(dtype).requires_grad_(grad) if a is not None else None  # noqa: E731
    x, res, w, b = t(c["x"], True), t(c["res"], True), t(c["w"], True), t(c["b"], True)
    rm, rv = t(c["rm"]), t(c["rv"])
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                      # the sums' order, and so the recorded units, must not depend on the core count
    try:
        tracked = c["tracked"]

        def call(xin):
            nonlocal tracked
            f = 0.0
            if c["training"] and rm is not None:
                tracked += 1
                f = br.momentum_factor(c["momentum"], tracked)
            return F.batch_norm(xin, rm, rv, w, b, c["batch_stats"], f, bm.EPS)

        z = call(x)
        if res is not None:
            z = z + res
        y = F.relu(z) if c["relu"] else z
        y.backward(t(c["g"]))
        out = {"y": y.detach().numpy(), "dx": x.grad.numpy()}
        if res is not None:
            out["dres"] = res.grad.numpy()
        if w is not None:
            out.update(dw=w.grad.numpy(), db=b.grad.numpy())
        if c["batch_stats"]:
            with torch.no_grad():
                out["mean"] = x.mean(dim=(0, 2)).numpy()
                out["invstd"] = (1.0 / torch.sqrt(x.var(dim=(0, 2), unbiased=False) + bm.EPS)).numpy()
        if c["calls"] == 2:
            with torch.no_grad():
                call(t(c["x2"]))
            out.update(rm=rm.numpy(), rv=rv.numpy())
    finally:
        torch.set_num_threads(threads)
    return out, tracked


def test_matrix_covers_what_it_says():
    names = bm.case_names()
    assert len(names) == len(set(names)) and set(bm.GOLDEN) <= set(names) and set(bm.GOLDEN) == set(bm.GOLDEN_SITE)
    shapes = [bm.CASES[n] for n in names]
    R, TL = br.ROWS, br.TILE
    assert {s[0] * s[1] for s in shapes} >= {1, 2, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 2 * R + 2}
    assert {s[2] for s in shapes} >= {1, 2, 3, 4, 5, 6, 7, TL - 1, TL, TL + 1, 2 * TL - 1, 2 * TL, 2 * TL + 1}
    assert any(s[0] * s[2] == 2 for s in shapes) and any(s[1] == 1 for s in shapes)
    assert {s[3:8] for s in shapes} == {(a, b, c, d, e) for a in (False, True) for b in (False, True) for c in (False, True)
                                        for d in (False, True) for e in (False, True)}
    assert {s[8] for s in shapes} == {0.1, 0.0, 1.0, None}
    n = {br.partials(s[0], s[2]) for s in shapes}
    assert any(v <= br.FOLD_SEGS for v in n) and any(v > br.FOLD_SEGS and v % br.fold_seg_len(v) == 1 for v in n)
    assert any(v > br.FOLD_SEGS and v % br.fold_seg_len(v) > 1 for v in n)
    assert bm.CASES["recipe_tcn"][:3] == (256, 64, 100) and bm.CASES["recipe_mdtc"][:3] == (100, 32, 200)
    assert sorted(s[0] * s[1] * s[2] for s in shapes)[-3] < 1 << 14                # the two recipes are the only large cases
    for name in ("off65536", "off4096"):
        c = bm.load_case(name)
        m = c["x"][:, 1::2].mean()
        assert abs(m - float(name[3:])) < 1.0 and 0.5 < c["x"][:, 1::2].std() < 1.5 and 111 <= c["x"].shape[0] * c["x"].shape[2] <= 3200
    c = bm.load_case("const")
    assert (c["x"][:, 2] == 3.25).all() and bm.oracle("const")[0]["invstd"][2] == 1.0 / np.sqrt(bm.EPS)
    for name in ("orth", "orth_relu"):
        ref, mag = bm.backward_oracle(name)
        assert np.all(np.abs(ref["db"]) <= 2.0 ** -12 * mag["db"]) and np.all(np.abs(ref["dw"]) <= 2.0 ** -12 * mag["dw"])
    assert np.all(np.abs(ref["db"]) <= 2.0 ** -12 * mag["db"]) and np.all(np.abs(ref["dw"]) <= 2.0 ** -12 * mag["dw"])
    for name in names:
        assert br.check(*bm.CASES[name][:3]), name
    for name in ("g_nonfinite_x", "g_nonfinite_g", "g_nonfinite_res"):
        key = {"g_nonfinite_x": "x", "g_nonfinite_g": "g", "g_nonfinite_res": "res"}[name]
        a = bm.load_case(name)[key]
        assert np.isnan(a[:, 1]).any() and np.isposinf(a[:, 3]).any() and np.isneginf(a[:, 5]).any() and np.isfinite(a[:, 0::2][:, :2]).all()


def golden_oracle(name):
    """The oracle's quantities as the goldens record them: one call, the gradients on the float64 statistics themselves."""
    c = bm.load_case(name)
    B, _, T = c["x"].shape
    N = B * T
    ref, mag, _ = bm.oracle(name)
    out, m = {"y": ref["y"]}, {"y": mag["y"]}
    if c["batch_stats"]:
        st, _ = br.batch_stats(c["x"], bm.EPS)
    else:
        st, _ = br.eval_stats(c["rm"], c["rv"], bm.EPS)
    r, rmag = br.backward(c["x"], ref["y"], c["g"], c["w"], st["mean"], st["invstd"], c["batch_stats"], c["relu"])
    if c["res"] is None:
        del r["dres"]
    out.update(r)
    m.update(rmag)
    tracked = c["tracked"]
    if c["training"]:
        tracked += 1
        f = br.momentum_factor(c["momentum"], tracked)
        out["rm"], m["rm"] = br.running_update(c["rm"], st["mean"], f)
        out["rv"], m["rv"] = br.running_update(c["rv"], st["var"] * (N / (N - 1.0)), f)
    else:
        out["rm"], m["rm"] = c["rm"].astype(np.float64), np.abs(c["rm"]).astype(np.float64)
        out["rv"], m["rv"] = c["rv"].astype(np.float64), np.abs(c["rv"]).astype(np.float64)
    return out, m, tracked


@pytest.mark.parametrize("name", sorted(bm.GOLDEN))
def test_oracle_equals_the_reference_in_float64(golden, name):
    c = bm.load_case(name)
    for k in ("x", "g", "res", "w", "b", "rm", "rv"):
        if c[k] is not None:
            assert np.array_equal(golden[f"{name}/{k}"], c[k], equal_nan=True)       # the golden was made from these inputs
        else:
            assert f"{name}/{k}" not in golden
    ref, mag, tracked = golden_oracle(name)
    assert int(golden[f"{name}/tracked64"]) == tracked == int(golden[f"{name}/tracked32"])
    for k in ref:
        want = golden[f"{name}/{k}64"]
        assert bm.same_classes(ref[k], want), (name, k)
        fin = np.isfinite(want)
        dev = np.abs(ref[k][fin] - want[fin])
        assert np.all(dev <= 1e-12 * mag[k][fin]), (name, k, float(dev.max()))
        assert bm.same_classes(golden[f"{name}/{k}32"], want), (name, k)             # and the float32 reference has its classes


def test_classes_the_goldens_pin(golden):
    """What the reference does with non-finite values, from its own float64 and float32 runs."""
    for tag in ("32", "64"):
        y, dx, dw, db, dres = (golden[f"g_nonfinite_x/{k}{tag}"] for k in ("y", "dx", "dw", "db", "dres"))
        # a NaN or an Inf anywhere in a channel: its whole output is NaN, the other channels are untouched
        assert np.isnan(y[:, 1::2]).all() and np.isfinite(y[:, 0::2]).all()
        assert np.isnan(dx[:, 1::2]).all() and np.isfinite(dx[:, 0::2]).all() and np.isnan(dw[1::2]).all() and np.isfinite(dw[0::2]).all()
        # the ReLU's backward passes the gradient where y is NaN: grad_residual is grad_y there, grad_bias its finite sum
        g = golden["g_nonfinite_x/g"]
        assert np.array_equal(dres[:, 1::2], g[:, 1::2].astype(dres.dtype)) and np.isfinite(db).all()
        rm, rv = golden[f"g_nonfinite_x/rm{tag}"], golden[f"g_nonfinite_x/rv{tag}"]
        assert np.isnan(rm[1]) and np.isposinf(rm[3]) and np.isneginf(rm[5]) and np.isnan(rv[1::2]).all() and np.isfinite(rv[0::2]).all()
        # eval: the statistics are the buffers', so only the element itself is hit
        y = golden[f"g_nonfinite_x_eval/y{tag}"]
        assert np.isnan(y[0, 1, 3]) and np.isfinite(y).sum() >= y.size - 3
        # a NaN in the residual: that element of y alone, and the gradient passes there
        y, dres = golden[f"g_nonfinite_res/y{tag}"], golden[f"g_nonfinite_res/dres{tag}"]
        assert np.isnan(y[0, 1, 3]) and np.isposinf(y[1, 3, 7]) and y[0, 5, 2] == 0 and np.isfinite(y).sum() == y.size - 2
        g = golden["g_nonfinite_res/g"]
        assert dres[0, 1, 3] == g[0, 1, 3] and dres[1, 3, 7] == g[1, 3, 7] and dres[0, 5, 2] == 0
        # a NaN in grad_y: its channel's parameter gradients and grad_x, that element of grad_residual
        dx, db, dres = (golden[f"g_nonfinite_g/{k}{tag}"] for k in ("dx", "db", "dres"))
        assert np.isnan(dx[:, 1]).all() and not np.isfinite(dx[:, 3::2]).any() and np.isfinite(dx[:, 0::2]).all()
        assert np.isnan(db[1]) and np.isposinf(db[3]) and np.isneginf(db[5])
        assert np.isnan(dres[0, 1, 3]) and np.isfinite(dres).sum() == dres.size - 3


@pytest.mark.parametrize("name", sorted(bm.GOLDEN))
def test_torch_path_equals_the_reference_bit_for_bit(golden, name):
    got, tracked = torch_path(name)
    assert np.array_equal(got["y"].view(np.int32), golden[f"{name}/y32"].view(np.int32)), name
    for k in ("dx", "dw", "db"):
        assert np.array_equal(got[k], golden[f"{name}/{k}32"], equal_nan=True), (name, k)
    u, bad = bm.units(name, got)
    assert not bad and all(u[k] <= bm.BARS[k] for k in u), (name, u, bad)             # the live reference is within its own bars


def bar(units):
    return pow2_at_or_above(4 * units) if units > 0 else 0.0          # (grad_residual is a copy or a zero: exact)


def test_bars_are_recomputed():
    worst = {k: (0.0, "") for k in bm.QUANTITIES}
    for name in bm.case_names():
        got, tracked = torch_path(name)
        assert tracked == bm.oracle(name)[2], name
        u, bad = bm.units(name, got)
        assert not bad, (name, bad)
        for k, v in u.items():
            if v > worst[k][0]:
                worst[k] = (v, name)
    for k in bm.QUANTITIES:
        print(f"{k}: reference's worst units {worst[k][0]:.2f} ({worst[k][1]}) -> bar {bar(worst[k][0])}")
    for k in bm.QUANTITIES:
        assert abs(worst[k][0] - bm.REF_UNITS[k]) <= 0.01 * max(1.0, bm.REF_UNITS[k]), (k, worst[k], bm.REF_UNITS[k])
        assert bm.BARS[k] == bar(bm.REF_UNITS[k]) == bar(worst[k][0]), (k, worst[k], bm.BARS[k])


def test_plain_sums_of_squares_miss_the_statistics_bound():
    """The check the shifted sums are for: var = E[x^2] - mean^2 in double, rounded once, is outside device_sum_bound on the
    offset channels; sums of x minus the channel's first element are inside it."""
    for name in ("off65536", "off4096"):
        c = bm.load_case(name)
        x = c["x"].astype(np.float64)
        N = x.shape[0] * x.shape[2]
        ref, _ = br.batch_stats(c["x"], bm.EPS)
        plain = (x ** 2).sum(axis=(0, 2)) / N - (x.sum(axis=(0, 2)) / N) ** 2
        d = x - x[:1, :, :1]
        s1, s2 = d.sum(axis=(0, 2)), (d ** 2).sum(axis=(0, 2))
        shifted = (s2 - s1 * s1 / N) / N
        u = lambda v: np.abs(f32v(v) - ref["var"]) / (bm.U * ref["var"])  # noqa: E731
        f32v = lambda v: v.astype(np.float32).astype(np.float64)  # noqa: E731
        print(f"{name}: var units plain {u(plain)[1::2].max():.2f} shifted {u(shifted)[1::2].max():.2f}")
        assert u(shifted).max() <= bm.device_sum_bound(name)
        if name == "off65536":
            assert u(plain)[1::2].max() > bm.device_sum_bound(name)


def test_workspace_size_and_plan_without_a_device():
    lib = _capi.load()
    for name in bm.case_names():
        args = bm.CASES[name][:3]
        assert lib.wekws_hip_batchnorm_workspace_bytes(*args) == br.workspace_bytes(*args) > 0, name
    assert br.workspace_bytes(256, 64, 100) == 256 * 64 * 16 + 64 * 8 + 16
    assert br.workspace_bytes(100, 32, 200) == 200 * 32 * 16 + 32 * 8 + 16
    assert br.workspace_bytes(1, 1, 1) == 16 + 16 + 16
    # 64-bit sizes: 2^16 batch rows of two tiles and 2^14 channels -> 2^35 bytes of partials
    assert lib.wekws_hip_batchnorm_workspace_bytes(1 << 16, 1 << 14, 129) == (1 << 35) + (1 << 17) + 16
    for bad in ((0, 5, 9), (2, 0, 9), (2, 5, 0), (-1, 5, 9), (1 << 20, 1 << 20, 1 << 20)):
        assert lib.wekws_hip_batchnorm_workspace_bytes(*bad) == 0 and _capi.last_error() != "", bad
        assert not br.check(*bad), bad
    assert br.fold_seg_len(9) == 2 and br.fold_seg_len(15) == 2 and br.fold_seg_len(20) == 3 and br.fold_seg_len(8) == 1


def test_every_refusal_holds_without_a_device():
    """Argument errors return EINVAL with a message before any launch: nothing here needs (or touches) a device, so the
    pointers are host addresses that are never dereferenced."""
    lib = _capi.load()
    buf = np.zeros(4096, np.float64)
    p = buf.ctypes.data
    assert p % 16 == 0
    nb = br.workspace_bytes(2, 5, 9)

    def fwd(x=p, res=p, B=2, C=5, T=9, w=p, b=p, rm=p, rv=p, nbt=p, batch=1, mom=0.1, eps=1e-5, relu=1, y=p, sm=p, si=p, ws=p, n=nb):
        return lib.wekws_hip_batchnorm_forward(x, res, B, C, T, w, b, rm, rv, nbt, batch, mom, eps, relu, y, sm, si, ws, n, None)

    def bwd(x=p, y=p, g=p, B=2, C=5, T=9, w=p, sm=p, si=p, batch=1, relu=1, dx=p, dres=p, dw=p, db=p, ws=p, n=nb):
        return lib.wekws_hip_batchnorm_backward(x, y, g, B, C, T, w, sm, si, batch, relu, dx, dres, dw, db, ws, n, None)

    def refused(rc, *words):
        return rc == -1 and all(w in _capi.last_error() for w in words) and _capi.last_error() != ""

    shape_errors = [dict(B=0), dict(C=0), dict(T=0), dict(B=-3), dict(C=-1), dict(T=-7), dict(B=1 << 20, C=1 << 20, T=1 << 20)]
    for call, nulls in ((fwd, ("x", "y", "sm", "si")), (bwd, ("x", "g", "sm", "si"))):
        for k in nulls:
            assert refused(call(**{k: None}), "NULL"), k
        for kw in shape_errors:
            assert refused(call(**kw)), kw
        assert refused(call(B=1, T=1), "more than one value") and refused(call(B=1, C=7, T=1), "more than one value")
        assert refused(call(ws=None), "workspace") and refused(call(ws=p + 8), "aligned") and refused(call(n=nb - 1), "workspace")
        assert refused(call(n=0))
    assert refused(fwd(B=1 << 20, C=1 << 20, T=1 << 20), "too large")
    assert refused(fwd(batch=0, rm=None, rv=None), "running")                         # eval without running buffers
    assert refused(fwd(rm=None), "both or neither") and refused(fwd(rv=None), "both or neither")
    assert refused(fwd(eps=0.0), "eps") and refused(fwd(eps=-1e-5), "eps") and refused(fwd(eps=float("nan")), "eps")
    assert refused(fwd(mom=1.5), "momentum") and refused(fwd(mom=float("nan")), "momentum")
    assert refused(fwd(mom=-1.0, nbt=None), "num_batches_tracked")
    assert refused(bwd(y=None), "needs y")
    # the workspace is needed for the parameter gradients in either mode, and for grad_x under batch statistics alone
    assert refused(bwd(batch=0, ws=None), "workspace") and refused(bwd(dx=None, dres=None, db=None, ws=None), "workspace")
    assert refused(bwd(dw=None, db=None, dres=None, ws=None), "workspace")
    assert not buf.any()
