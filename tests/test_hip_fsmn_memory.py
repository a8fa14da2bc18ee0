"""GPU: the FSMN memory block's kernels (wekws_hip_fsmn_memory_forward / _backward) on the case matrix of
tests/fsmn_memory_matrix.py: y, dx, dwl and dwr within the derived bars of the float64 oracle, non-finite classes, the same bits
on every run, in any batch position and beside an MFMA tenant, misaligned bases, optional outputs, refusals that launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fsmn_memory_matrix as fm
from tests import fsmn_memory_ref as fr
from tests.test_hip_tenants import tenant  # noqa: F401  (the MFMA tenants of the second stream)
from wekws_amd import _capi

pytestmark = pytest.mark.gpu

CANARY = -777.25


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def forward(x, wl, wr, lstride, rstride, y=None):
    B, T, D = x.shape
    y = torch.full_like(x, CANARY) if y is None else y
    rc = _capi.load().wekws_hip_fsmn_memory_forward(x.data_ptr(), B, T, D, wl.data_ptr(), wl.shape[1], lstride, wr.data_ptr(), wr.shape[1],
                                                    rstride, y.data_ptr(), _stream())
    assert rc == 0, _capi.last_error()
    return y


def backward(x, g, wl, wr, lstride, rstride, want_x=True, want_w=True):
    B, T, D = x.shape
    lib = _capi.load()
    dx = torch.full_like(x, CANARY) if want_x else None
    dwl = torch.full_like(wl, CANARY) if want_w else None
    dwr = torch.full_like(wr, CANARY) if want_w else None
    nb = lib.wekws_hip_fsmn_memory_workspace_bytes(B, T, D, wl.shape[1], wr.shape[1])
    assert nb == fr.workspace_bytes(B, T, D, wl.shape[1], wr.shape[1])
    ws = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device="cuda") if want_w else None
    rc = lib.wekws_hip_fsmn_memory_backward(x.data_ptr(), g.data_ptr(), B, T, D, wl.data_ptr(), wl.shape[1], lstride, wr.data_ptr(),
                                            wr.shape[1], rstride, dx.data_ptr() if want_x else None, dwl.data_ptr() if want_w else None,
                                            dwr.data_ptr() if want_w else None, ws.data_ptr() if want_w else None, nb if want_w else 0,
                                            _stream())
    assert rc == 0, _capi.last_error()
    return dx, dwl, dwr


def dev(c):
    return {k: torch.from_numpy(c[k].copy()).cuda() for k in ("x", "g", "wl", "wr")}


def run_case(name):
    c = fm.load_case(name)
    d = dev(c)
    got = {"y": forward(d["x"], d["wl"], d["wr"], c["lstride"], c["rstride"])}
    if c["backward"]:
        got["dx"], got["dwl"], got["dwr"] = backward(d["x"], d["g"], d["wl"], d["wr"], c["lstride"], c["rstride"])
    return got


def bits(t):
    return t.view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


@pytest.mark.parametrize("name", fm.case_names())
def test_matrix_within_the_bars(name, error_report):
    got = run_case(name)
    u, bad = fm.units(name, {k: v.cpu().numpy() for k, v in got.items()})
    print(f"{name}: device units " + " ".join(f"{k} {v:.3f}" for k, v in u.items()))
    for k, v in u.items():
        key = f"fsmn_memory/{k}"
        if v >= error_report.get(key, (-1.0, ""))[0]:
            error_report[key] = (v, name)
    assert not bad, (name, "classes differ", bad)
    for k, v in u.items():
        assert v <= fm.BARS[k], (name, k, v)
        if k in ("dwl", "dwr"):
            assert v <= fm.device_dw_bound(name), (name, k, v, fm.device_dw_bound(name))
    assert same(got, run_case(name)), name                                       # two runs, the same bits


def test_first_frames_are_nan_under_an_inf_tap():
    c = fm.load_case("g_inf_tap")
    y = run_case("g_inf_tap")["y"].cpu().numpy()
    ref, _ = fm.oracle("g_inf_tap")
    assert fm.same_classes(y, ref["y"])
    # channel 1 holds an Inf in its tap of delay R = 2: frames 0 and 1 multiply it into the zeros before the row
    assert np.isnan(y[:, :2, 1]).all() and np.isfinite(y[:, :, 0]).all() and np.isfinite(y[:, :, 3]).all()
    assert c["wl"][1, -1] == np.inf


def test_classes_with_nonfinite_frames():
    got = run_case("g_nonfinite_x")
    ref, _ = fm.oracle("g_nonfinite_x")
    for k, v in got.items():
        assert fm.same_classes(v.cpu().numpy(), ref[k]), k
    assert np.isnan(ref["y"]).any() and np.isinf(ref["y"]).any() and np.isfinite(ref["dx"]).all() and np.isnan(ref["dwl"]).all()


@pytest.mark.parametrize("D", [8, 5])
def test_rows_do_not_depend_on_their_batch(D):
    """Each row of a B = 5 call equals, bit for bit, the same row run alone and in a permuted batch: y and dx."""
    rng = np.random.default_rng(D)
    T, taps = 70, fm.RECIPE_TAPS
    x = torch.from_numpy(rng.standard_normal((5, T, D)).astype(np.float32)).cuda()
    g = torch.from_numpy(rng.standard_normal((5, T, D)).astype(np.float32)).cuda()
    wl = torch.from_numpy((0.3 * rng.standard_normal((D, taps[0]))).astype(np.float32)).cuda()
    wr = torch.from_numpy((0.3 * rng.standard_normal((D, taps[1]))).astype(np.float32)).cuda()
    y = forward(x, wl, wr, 1, 1)
    dx, _, _ = backward(x, g, wl, wr, 1, 1, want_w=False)
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    yp = forward(x[perm].contiguous(), wl, wr, 1, 1)
    dxp, _, _ = backward(x[perm].contiguous(), g[perm].contiguous(), wl, wr, 1, 1, want_w=False)
    assert torch.equal(bits(yp), bits(y[perm])) and torch.equal(bits(dxp), bits(dx[perm]))
    for b in range(5):
        y1 = forward(x[b:b + 1].contiguous(), wl, wr, 1, 1)
        dx1, _, _ = backward(x[b:b + 1].contiguous(), g[b:b + 1].contiguous(), wl, wr, 1, 1, want_w=False)
        assert torch.equal(bits(y1[0]), bits(y[b])) and torch.equal(bits(dx1[0]), bits(dx[b])), b


@pytest.mark.parametrize("name", ["d64", "t131_r", "fold9"])
def test_misaligned_bases_give_the_same_bits(name):
    """A base 4 bytes off a 16-byte boundary takes the scalar accesses: every result has the aligned run's bits."""
    c = fm.load_case(name)
    d = dev(c)
    want = run_case(name)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    xs, gs = shifted(d["x"]), shifted(d["g"])
    ys = shifted(torch.full_like(d["x"], CANARY))
    forward(xs, d["wl"], d["wr"], c["lstride"], c["rstride"], y=ys)
    dx, dwl, dwr = backward(xs, gs, d["wl"], d["wr"], c["lstride"], c["rstride"])
    assert same({"y": ys.contiguous(), "dx": dx, "dwl": dwl, "dwr": dwr}, want)
    # only one of the two tensors off the boundary
    dx2, dwl2, dwr2 = backward(d["x"], gs, d["wl"], d["wr"], c["lstride"], c["rstride"])
    assert same({"dx": dx2, "dwl": dwl2, "dwr": dwr2}, {k: want[k] for k in ("dx", "dwl", "dwr")})


def test_optional_outputs_leave_the_others_alone():
    c = fm.load_case("t65_r")
    d = dev(c)
    dx, dwl, dwr = backward(d["x"], d["g"], d["wl"], d["wr"], 1, 1)
    dx_only, a, b = backward(d["x"], d["g"], d["wl"], d["wr"], 1, 1, want_w=False)
    assert a is None and b is None and torch.equal(bits(dx_only), bits(dx))
    none, dwl_only, dwr_only = backward(d["x"], d["g"], d["wl"], d["wr"], 1, 1, want_x=False)
    assert none is None and torch.equal(bits(dwl_only), bits(dwl)) and torch.equal(bits(dwr_only), bits(dwr))


def test_refused_calls_launch_nothing():
    lib = _capi.load()
    c = fm.load_case("g_small")
    d = dev(c)
    B, T, D = d["x"].shape
    y = torch.full_like(d["x"], CANARY)
    dx = torch.full_like(d["x"], CANARY)
    dwl = torch.full_like(d["wl"], CANARY)
    dwr = torch.full_like(d["wr"], CANARY)
    nb = fr.workspace_bytes(B, T, D, 10, 2)
    ws = torch.full((nb // 8 + 2,), CANARY, dtype=torch.float64, device="cuda")
    p = {k: v.data_ptr() for k, v in d.items()}

    def fwd(x=p["x"], B=B, T=T, D=D, wl=p["wl"], lo=10, ls=1, wr=p["wr"], ro=2, rs=1, out=y.data_ptr()):
        return lib.wekws_hip_fsmn_memory_forward(x, B, T, D, wl, lo, ls, wr, ro, rs, out, _stream())

    def bwd(x=p["x"], g=p["g"], B=B, T=T, D=D, wl=p["wl"], lo=10, ls=1, wr=p["wr"], ro=2, rs=1, gx=dx.data_ptr(), gl=dwl.data_ptr(),
            gr=dwr.data_ptr(), w=ws.data_ptr(), n=nb):
        return lib.wekws_hip_fsmn_memory_backward(x, g, B, T, D, wl, lo, ls, wr, ro, rs, gx, gl, gr, w, n, _stream())

    for kw in (dict(x=None), dict(wl=None), dict(wr=None), dict(out=None), dict(B=0), dict(T=-1), dict(D=0), dict(lo=0), dict(ro=0),
               dict(ls=0), dict(rs=0), dict(lo=31, ro=2), dict(ls=29)):
        assert fwd(**kw) == -1 and _capi.last_error() != "", kw
    for kw in (dict(x=None), dict(g=None), dict(wl=None), dict(wr=None), dict(B=0), dict(T=0), dict(D=-2), dict(lo=0), dict(ro=0), dict(ls=0),
               dict(rs=-1), dict(lo=31, ro=2), dict(ls=29), dict(n=nb - 1), dict(w=None), dict(w=ws.data_ptr() + 8), dict(gl=None),
               dict(gr=None)):
        assert bwd(**kw) == -1 and _capi.last_error() != "", kw
    torch.cuda.synchronize()
    for t in (y, dx, dwl, dwr, ws):
        assert bool((t == CANARY).all())
    assert fwd() == 0 and bwd() == 0                                             # and the same buffers are written by a good call
    torch.cuda.synchronize()
    for t in (y, dx, dwl, dwr):
        assert not bool((t == CANARY).any())


def test_every_launch_beside_an_mfma_tenant(tenant):  # noqa: F811
    """The kernels on one stream, an MFMA-heavy forward on another: bit-identical to the solo run."""
    names = ["g_mid", "d5", "t259_r", "fold15", "t33_long", "recipe"]
    solo = [run_case(n) for n in names]
    tm, tx = tenant
    torch.cuda.synchronize()
    s_a, s_b = torch.cuda.Stream(), torch.cuda.Stream()
    for rnd in range(4):
        with torch.cuda.stream(s_b):
            for _ in range(5):
                tm(tx)
        with torch.cuda.stream(s_a):
            got = [run_case(n) for n in names]
        torch.cuda.synchronize()
        for n, a, b in zip(names, got, solo):
            assert same(a, b), (n, rnd)
