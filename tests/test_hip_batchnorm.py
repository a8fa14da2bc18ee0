"""GPU: the BatchNorm1d kernels (wekws_hip_batchnorm_forward / _backward) on the case matrix of tests/batchnorm_matrix.py: every
quantity within the derived bars of the float64 oracle and the sums within the bound of their own arithmetic, non-finite classes,
canaries around every output and past the workspace, the same bits on every run, for every subset of the gradients, for a channel
whatever the other channels, from misaligned bases and beside an MFMA tenant; a negative control; refusals that launch nothing."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import batchnorm_matrix as bm
from tests import batchnorm_ref as br
from tests.test_hip_tenants import tenant  # noqa: F401  (the MFMA tenants of the second stream)
from wekws_amd import _capi

pytestmark = pytest.mark.gpu

CANARY = -777.25
GUARD = 8                                        # canary floats on either side of every output
GRADS = ("dx", "dres", "dw", "db")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(shape, offset=0):
    """-> (buffer, view): a canary-filled float32 buffer and the view of `shape` that starts GUARD + offset floats into it.
    GUARD is a multiple of four, so offset = 0 keeps the 16-byte alignment and offset = 1 breaks it."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + 4,), CANARY, dtype=torch.float32, device="cuda")
    view = buf[GUARD + offset:GUARD + offset + n].view(shape)
    assert view.data_ptr() % 16 == 4 * offset
    return buf, view


def intact(buf, view):
    """The canaries around `view` are untouched and none is left inside it."""
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    hi = lo + view.numel()
    return bool((buf[:lo] == CANARY).all()) and bool((buf[hi:] == CANARY).all()) and not bool((view == CANARY).any())


def workspace(B, Cc, T):
    nb = _capi.load().wekws_hip_batchnorm_workspace_bytes(B, Cc, T)
    assert nb == br.workspace_bytes(B, Cc, T) and nb % 16 == 0
    return torch.full((nb // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda"), nb


def ptr(t):
    return t.data_ptr() if t is not None else None


def shifted(t, offset):
    """A copy of `t` whose base is 4 * offset bytes past a 16-byte boundary."""
    if t is None or offset == 0:
        return t
    _, v = guarded(t.shape, offset)
    v.copy_(t)
    return v


def forward(x, res, w, b, rm, rv, nbt, batch_stats, momentum, relu, offset=0):
    """One forward call.  rm, rv (guarded (buffer, view) pairs or None) and nbt ((3,) int64: a canary either side, or None) are
    updated in place.  -> dict(y, mean, invstd)."""
    B, Cc, T = x.shape
    out = {"y": guarded((B, Cc, T), offset), "mean": guarded((Cc,)), "invstd": guarded((Cc,))}
    ws, nb = workspace(B, Cc, T)
    rc = _capi.load().wekws_hip_batchnorm_forward(
        x.data_ptr(), ptr(res), B, Cc, T, ptr(w), ptr(b), ptr(rm[1]) if rm else None, ptr(rv[1]) if rv else None,
        nbt[1:].data_ptr() if nbt is not None else None, int(batch_stats), -1.0 if momentum is None else momentum, bm.EPS, int(relu),
        out["y"][1].data_ptr(), out["mean"][1].data_ptr(), out["invstd"][1].data_ptr(), ws.data_ptr() if batch_stats else None,
        nb if batch_stats else 0, _stream())
    assert rc == 0, _capi.last_error()
    for k, (buf, view) in out.items():
        assert intact(buf, view), k
    for k, pair in (("rm", rm), ("rv", rv)):
        assert pair is None or intact(*pair), k
    assert nbt is None or (int(nbt[0]) == -7 and int(nbt[2]) == -7)
    assert bool(torch.isnan(ws[nb // 8:]).all())                                 # nothing past the workspace's stated size
    return {k: v for k, (_, v) in out.items()}


def backward(x, y, g, w, mean, invstd, batch_stats, relu, want=GRADS, offset=0):
    B, Cc, T = x.shape
    shapes = {"dx": (B, Cc, T), "dres": (B, Cc, T), "dw": (Cc,), "db": (Cc,)}
    out = {k: guarded(shapes[k], offset if k in ("dx", "dres") else 0) for k in want}
    need_ws = "dw" in want or "db" in want or (batch_stats and "dx" in want)
    ws, nb = workspace(B, Cc, T)
    p = lambda k: out[k][1].data_ptr() if k in out else None  # noqa: E731
    rc = _capi.load().wekws_hip_batchnorm_backward(x.data_ptr(), ptr(y) if relu else None, g.data_ptr(), B, Cc, T, ptr(w), mean.data_ptr(),
                                                   invstd.data_ptr(), int(batch_stats), int(relu), p("dx"), p("dres"), p("dw"), p("db"),
                                                   ws.data_ptr() if need_ws else None, nb if need_ws else 0, _stream())
    assert rc == 0, _capi.last_error()
    for k, (buf, view) in out.items():
        assert intact(buf, view), k
    assert bool(torch.isnan(ws[nb // 8:]).all())
    return {k: v for k, (_, v) in out.items()}


def dev(c):
    return {k: torch.from_numpy(c[k].copy()).cuda() if c[k] is not None else None for k in ("x", "g", "x2", "res", "w", "b", "rm", "rv")}


def run_case(name, offset=0, want=None, channels=None):
    """The case's calls through the C ABI -> (dict of device tensors over the case's quantities, num_batches_tracked after).
    offset: x, g, the residual, y, dx and dres start 4 * offset bytes past a 16-byte boundary.  channels: the case restricted to
    (and in the order of) these channels."""
    c = bm.load_case(name)
    d = dev(c)
    if channels is not None:
        idx = torch.tensor(channels, device="cuda")
        d = {k: (v.index_select(1 if v.dim() == 3 else 0, idx).contiguous() if v is not None else None) for k, v in d.items()}
    x, g, x2, res = (shifted(d[k], offset) for k in ("x", "g", "x2", "res"))
    Cc = x.shape[1]
    rm = rv = nbt = None
    if d["rm"] is not None:
        rm, rv = guarded((Cc,)), guarded((Cc,))
        rm[1].copy_(d["rm"])
        rv[1].copy_(d["rv"])
        nbt = torch.tensor([-7, c["tracked"], -7], dtype=torch.int64, device="cuda")
    got = forward(x, res, d["w"], d["b"], rm, rv, nbt, c["batch_stats"], c["momentum"], c["relu"], offset)
    if c["calls"] == 2:
        forward(x2, res, d["w"], d["b"], rm, rv, nbt, True, c["momentum"], c["relu"], offset)
        got.update(rm=rm[1], rv=rv[1])
    elif rm is not None:                                                         # statistics from the buffers: nothing moves
        assert torch.equal(rm[1], d["rm"]) and torch.equal(rv[1], d["rv"]) and int(nbt[1]) == c["tracked"]
    if want is None:
        want = tuple(k for k in GRADS if k != "dres" or res is not None)
    got.update(backward(x, got["y"], g, d["w"], got["mean"], got["invstd"], c["batch_stats"], c["relu"], want, offset))
    return got, (int(nbt[1]) if nbt is not None else None)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return set(a) == set(b) and all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


def host(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize("name", bm.case_names())
def test_matrix_within_the_bars(name, error_report):
    got, tracked = run_case(name)
    h = host(got)
    u, bad = bm.units(name, h, saved=(h["mean"], h["invstd"]))
    print(f"{name}: device units " + " ".join(f"{k} {v:.3f}" for k, v in u.items()))
    for k, v in u.items():
        key = f"batchnorm/{k}"
        if v >= error_report.get(key, (-1.0, ""))[0]:
            error_report[key] = (v, name)
    assert not bad, (name, "classes differ", bad)
    assert tracked == bm.oracle(name)[2], name
    for k, v in u.items():
        assert v <= bm.BARS[k], (name, k, v)
        if k in bm.SUMS:
            assert v <= bm.device_sum_bound(name), (name, k, v, bm.device_sum_bound(name))
    again, tracked2 = run_case(name)
    assert same(got, again) and tracked2 == tracked, name                        # two runs, the same bits


def test_classes_with_nonfinite_values():
    for name in ("g_nonfinite_x", "g_nonfinite_x_eval", "g_nonfinite_g", "g_nonfinite_res"):
        h = host(run_case(name)[0])
        _, bad = bm.units(name, h, saved=(h["mean"], h["invstd"]))
        assert not bad, (name, bad)
    h = host(run_case("g_nonfinite_x")[0])
    # a NaN or an Inf in a channel: its statistics and outputs, and no other channel's; the ReLU's backward passes where y is NaN
    assert np.isnan(h["y"][:, 1::2]).all() and np.isfinite(h["y"][:, 0::2]).all() and np.isnan(h["dx"][:, 1::2]).all()
    assert np.isnan(h["mean"][1]) and np.isposinf(h["mean"][3]) and np.isneginf(h["mean"][5]) and np.isnan(h["invstd"][1::2]).all()
    assert np.isnan(h["rm"][1]) and np.isposinf(h["rm"][3]) and np.isneginf(h["rm"][5]) and np.isnan(h["rv"][1::2]).all()
    assert np.isfinite(h["db"]).all() and np.isnan(h["dw"][1::2]).all() and np.isfinite(h["dw"][0::2]).all()
    assert np.array_equal(h["dres"][:, 1::2], bm.load_case("g_nonfinite_x")["g"][:, 1::2])


def test_a_constant_channel_is_exact():
    h = host(run_case("const")[0])
    c = bm.load_case("const")
    assert h["mean"][2] == 3.25 and h["invstd"][2] == np.float32(1.0 / np.sqrt(bm.EPS))
    z = c["b"][2] + c["res"][:, 2]                                               # (x - mean) is an exact zero: y is bias + residual
    assert np.array_equal(h["y"][:, 2], np.where(z < 0, np.float32(0), z))


@pytest.mark.parametrize("name", ["t129", "f11111", "f01011", "fold9", "f10010"])
def test_every_subset_of_the_gradients_has_the_full_calls_bits(name):
    full, _ = run_case(name)
    have = tuple(k for k in GRADS if k in full)
    for n in range(len(have)):
        for want in itertools.combinations(have, n):
            part, _ = run_case(name, want=want)
            assert set(part) & set(GRADS) == set(want) and same({k: part[k] for k in want}, {k: full[k] for k in want}), want


@pytest.mark.parametrize("name", ["t6", "t129", "off65536", "g_nonfinite_x", "f01111"])
def test_a_channel_does_not_depend_on_the_others(name):
    """Every channel alone, and the channels in another order, have the bits they have in the full call."""
    full, _ = run_case(name)
    Cc = bm.CASES[name][1]
    perm = [(3 * i + 1) % Cc for i in range(Cc)] if Cc % 3 else list(range(Cc))[::-1]
    for channels in [perm] + [[c] for c in range(Cc)]:
        part, _ = run_case(name, channels=channels)
        idx = torch.tensor(channels, device="cuda")
        assert same(part, {k: v.index_select(1 if v.dim() == 3 else 0, idx) for k, v in full.items()}), channels


@pytest.mark.parametrize("name", ["t4", "t128", "t256", "f11110", "f11010", "eval8", "recipe_mdtc"])
def test_misaligned_bases_give_the_same_bits(name):
    """Rows of a multiple of four frames take the 16-byte accesses from aligned bases; a base 4 bytes off a 16-byte boundary
    takes the scalar ones: every result has the aligned run's bits."""
    assert bm.CASES[name][2] % 4 == 0
    want, _ = run_case(name)
    got, _ = run_case(name, offset=1)
    assert same(got, want)
    # only one tensor of a call off the boundary
    c = bm.load_case(name)
    d = dev(c)
    for k in ("x", "res"):
        if d[k] is None:
            continue
        t = {**d, k: shifted(d[k], 1)}
        y = forward(t["x"], t["res"], d["w"], d["b"], None, None, None, True, c["momentum"], c["relu"])["y"] if c["batch_stats"] else None
        assert y is None or torch.equal(bits(y), bits(want["y"])), k
    for k in ("x", "g", "y"):
        t = {"x": d["x"], "g": d["g"], "y": want["y"]}
        t[k] = shifted(t[k], 1)
        grads = backward(t["x"], t["y"], t["g"], d["w"], want["mean"], want["invstd"], c["batch_stats"], c["relu"],
                         tuple(k2 for k2 in GRADS if k2 in want))
        assert same(grads, {k2: want[k2] for k2 in grads}), k


def test_fp16_weights_miss_the_y_bar():
    """The negative control: the recipe case with its weight rounded to fp16 is outside the bar the float32 weight is held to."""
    c = bm.load_case("recipe_tcn")
    d = dev(c)
    y = forward(d["x"], None, d["w"].half().float(), d["b"], None, None, None, True, 0.1, True)["y"]
    u, bad = bm.units("recipe_tcn", {"y": y.cpu().numpy()})
    print(f"fp16 weight: y {u['y']:.1f} units (bar {bm.BARS['y']})")
    assert not bad and u["y"] > bm.BARS["y"]


def test_refused_calls_launch_nothing():
    lib = _capi.load()
    c = bm.load_case("g_bn2")
    d = dev(c)
    B, Cc, T = c["x"].shape
    full = lambda shape: torch.full(shape, CANARY, device="cuda")  # noqa: E731
    y, dx, dres = full((B, Cc, T)), full((B, Cc, T)), full((B, Cc, T))
    sm, si, dw, db = full((Cc,)), full((Cc,)), full((Cc,)), full((Cc,))
    rm, rv = d["rm"].clone(), d["rv"].clone()
    nbt = torch.tensor([5], dtype=torch.int64, device="cuda")
    nb = br.workspace_bytes(B, Cc, T)
    ws = torch.full((nb // 8 + 2,), CANARY, dtype=torch.float64, device="cuda")
    p = {k: v.data_ptr() for k, v in d.items() if v is not None}
    mean, invstd = torch.zeros(Cc, device="cuda"), torch.ones(Cc, device="cuda")

    def fwd(x=p["x"], res=p["res"], B=B, C=Cc, T=T, rmp=rm.data_ptr(), rvp=rv.data_ptr(), nbtp=nbt.data_ptr(), batch=1, mom=0.1, eps=1e-5,
            out=y.data_ptr(), wsp=ws.data_ptr(), n=nb):
        return lib.wekws_hip_batchnorm_forward(x, res, B, C, T, p["w"], p["b"], rmp, rvp, nbtp, batch, mom, eps, 1, out, sm.data_ptr(),
                                               si.data_ptr(), wsp, n, _stream())

    def bwd(x=p["x"], yp=d["x"].data_ptr(), g=p["g"], B=B, C=Cc, T=T, batch=1, relu=1, gx=dx.data_ptr(), gr=dres.data_ptr(),
            gw=dw.data_ptr(), gb=db.data_ptr(), wsp=ws.data_ptr(), n=nb):
        return lib.wekws_hip_batchnorm_backward(x, yp, g, B, C, T, p["w"], mean.data_ptr(), invstd.data_ptr(), batch, relu, gx, gr, gw, gb,
                                                wsp, n, _stream())

    for kw in (dict(x=None), dict(out=None), dict(B=0), dict(C=-1), dict(T=0), dict(B=1, T=1), dict(batch=0, rmp=None, rvp=None),
               dict(rmp=None), dict(eps=0.0), dict(mom=1.25), dict(mom=-1.0, nbtp=None), dict(wsp=None), dict(wsp=ws.data_ptr() + 8),
               dict(n=nb - 1)):
        assert fwd(**kw) == -1 and _capi.last_error() != "", kw
    for kw in (dict(x=None), dict(g=None), dict(yp=None), dict(B=0), dict(C=0), dict(T=-2), dict(B=1, T=1), dict(n=nb - 1), dict(wsp=None),
               dict(wsp=ws.data_ptr() + 8), dict(batch=0, wsp=None), dict(gw=None, gb=None, gr=None, n=0)):
        assert bwd(**kw) == -1 and _capi.last_error() != "", kw
    torch.cuda.synchronize()
    for t in (y, dx, dres, sm, si, dw, db, ws):
        assert bool((t == CANARY).all())
    assert torch.equal(rm, d["rm"]) and torch.equal(rv, d["rv"]) and int(nbt) == 5
    assert fwd() == 0 and bwd() == 0                                             # and the same buffers are written by a good call
    # what a call does not need it does not ask for: no workspace for the buffers' statistics, nor for grad_x alone under them
    assert fwd(batch=0, wsp=None, n=0) == 0 and bwd(batch=0, gw=None, gb=None, wsp=None, n=0) == 0
    assert bwd(relu=0, yp=None) == 0
    torch.cuda.synchronize()
    for t in (y, dx, dres, sm, si, dw, db):
        assert not bool((t == CANARY).any())
    assert int(nbt) == 6 and not torch.equal(rm, d["rm"])


def test_every_launch_beside_an_mfma_tenant(tenant):  # noqa: F811
    """The kernels on one stream, an MFMA-heavy forward on another: bit-identical to the solo run."""
    names = ["g_bn2", "r17", "t257", "fold15", "f11011", "eval8", "off65536", "recipe_tcn", "recipe_mdtc"]
    solo = [run_case(n)[0] for n in names]
    tm, tx = tenant
    torch.cuda.synchronize()
    s_a, s_b = torch.cuda.Stream(), torch.cuda.Stream()
    for rnd in range(4):
        with torch.cuda.stream(s_b):
            for _ in range(5):
                tm(tx)
        with torch.cuda.stream(s_a):
            got = [run_case(n)[0] for n in names]
        torch.cuda.synchronize()
        for n, a, b in zip(names, got, solo):
            assert same(a, b), (n, rnd)
