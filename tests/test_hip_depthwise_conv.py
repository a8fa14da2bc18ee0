"""GPU: the depthwise Conv1d kernels (wekws_hip_depthwise_conv1d_forward / _backward) on the case matrix of
tests/depthwise_conv_matrix.py: y, dx, dw and db within the derived bars of the float64 oracle, non-finite classes, canaries
around every output, the same bits on every run, for every subset of the gradients, in any batch position, from misaligned
bases, beside an MFMA tenant and for left_pad against an explicitly padded input; a negative control; refusals that launch
nothing."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import depthwise_conv_matrix as dm
from tests import depthwise_conv_ref as dr
from tests.test_hip_tenants import tenant  # noqa: F401  (the MFMA tenants of the second stream)
from wekws_amd import _capi

pytestmark = pytest.mark.gpu

CANARY = -777.25
GUARD = 8                                        # canary floats on either side of every output


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


def forward(x, w, bias, d, P, offset=0):
    B, Cc, Tin = x.shape
    K = w.shape[1]
    buf, y = guarded((B, Cc, dr.tout(Tin, K, d, P)), offset)
    rc = _capi.load().wekws_hip_depthwise_conv1d_forward(x.data_ptr(), B, Cc, Tin, w.data_ptr(), bias.data_ptr() if bias is not None else None,
                                                         K, d, P, y.data_ptr(), _stream())
    assert rc == 0, _capi.last_error()
    assert intact(buf, y)
    return y


def backward(x, g, w, d, P, want=("dx", "dw", "db"), offset=0):
    B, Cc, Tin = x.shape
    K = w.shape[1]
    lib = _capi.load()
    shapes = {"dx": (B, Cc, Tin), "dw": (Cc, K), "db": (Cc,)}
    out = {k: guarded(shapes[k], offset if k == "dx" else 0) for k in want}
    nb = lib.wekws_hip_depthwise_conv1d_workspace_bytes(B, Cc, Tin, K, d, P)
    assert nb == dr.workspace_bytes(B, Cc, Tin, K, d, P)
    need_ws = "dw" in want or "db" in want
    ws = torch.full((nb // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda") if need_ws else None
    ptr = lambda k: out[k][1].data_ptr() if k in out else None  # noqa: E731
    rc = lib.wekws_hip_depthwise_conv1d_backward(x.data_ptr(), g.data_ptr(), B, Cc, Tin, w.data_ptr(), K, d, P, ptr("dx"), ptr("dw"), ptr("db"),
                                                 ws.data_ptr() if need_ws else None, nb if need_ws else 0, _stream())
    assert rc == 0, _capi.last_error()
    for k, (buf, view) in out.items():
        assert intact(buf, view), k
    if need_ws:
        assert bool(torch.isnan(ws[nb // 8:]).all())                             # nothing past the workspace's stated size
    return {k: v for k, (_, v) in out.items()}


def dev(c):
    return {k: torch.from_numpy(c[k].copy()).cuda() if c[k] is not None else None for k in ("x", "g", "w", "bias")}


def run_case(name):
    c = dm.load_case(name)
    d = dev(c)
    got = {"y": forward(d["x"], d["w"], d["bias"], c["d"], c["P"])}
    if c["backward"]:
        got.update(backward(d["x"], d["g"], d["w"], c["d"], c["P"]))
    return got


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


@pytest.mark.parametrize("name", dm.case_names())
def test_matrix_within_the_bars(name, error_report):
    got = run_case(name)
    u, bad = dm.units(name, {k: v.cpu().numpy() for k, v in got.items()})
    print(f"{name}: device units " + " ".join(f"{k} {v:.3f}" for k, v in u.items()))
    for k, v in u.items():
        key = f"depthwise_conv/{k}"
        if v >= error_report.get(key, (-1.0, ""))[0]:
            error_report[key] = (v, name)
    assert not bad, (name, "classes differ", bad)
    for k, v in u.items():
        assert v <= dm.BARS[k], (name, k, v)
        if k in ("dw", "db"):
            assert v <= dm.device_dw_bound(name), (name, k, v, dm.device_dw_bound(name))
    assert same(got, run_case(name)), name                                       # two runs, the same bits


def test_first_frames_are_nan_under_an_inf_tap():
    c = dm.load_case("g_inf_tap")
    y = run_case("g_inf_tap")["y"].cpu().numpy()
    ref, _ = dm.oracle("g_inf_tap")
    assert dm.same_classes(y, ref["y"])
    # channel 1 holds an Inf in tap 0, which reads the P frames of padding in front of the row: Inf * 0
    assert np.isnan(y[:, 1, :c["P"]]).all() and np.isinf(y[:, 1, c["P"]:]).all() and np.isfinite(y[:, 0]).all() and np.isfinite(y[:, 3]).all()
    assert c["w"][1, 0] == np.inf and c["P"] > 0


def test_classes_with_nonfinite_samples():
    got = run_case("g_nonfinite_x")
    ref, _ = dm.oracle("g_nonfinite_x")
    for k, v in got.items():
        assert dm.same_classes(v.cpu().numpy(), ref[k]), k
    assert np.isnan(ref["y"]).any() and np.isinf(ref["y"]).any() and np.isfinite(ref["dx"]).all() and np.isnan(ref["dw"]).any()


@pytest.mark.parametrize("name", ["t129_k8d8", "len23", "fold9"])
def test_every_subset_of_the_gradients_has_the_full_calls_bits(name):
    c = dm.load_case(name)
    d = dev(c)
    full = backward(d["x"], d["g"], d["w"], c["d"], c["P"])
    for n in (1, 2):
        for want in itertools.combinations(("dx", "dw", "db"), n):
            part = backward(d["x"], d["g"], d["w"], c["d"], c["P"], want=want)
            assert set(part) == set(want) and same(part, {k: full[k] for k in want}), want
    # nothing wanted: nothing launched, no workspace needed
    assert backward(d["x"], d["g"], d["w"], c["d"], c["P"], want=()) == {}


@pytest.mark.parametrize("T", [72, 70])
def test_rows_do_not_depend_on_their_batch(T):
    """Each row of a B = 5 call equals, bit for bit, the same row run alone and in a permuted batch: y and dx."""
    rng = np.random.default_rng(T)
    Cc, K, d, P = 3, 8, 8, 56
    x = torch.from_numpy(rng.standard_normal((5, Cc, T)).astype(np.float32)).cuda()
    g = torch.from_numpy(rng.standard_normal((5, Cc, T)).astype(np.float32)).cuda()
    w = torch.from_numpy((0.3 * rng.standard_normal((Cc, K))).astype(np.float32)).cuda()
    b = torch.from_numpy((0.3 * rng.standard_normal(Cc)).astype(np.float32)).cuda()
    y = forward(x, w, b, d, P)
    dx = backward(x, g, w, d, P, want=("dx",))["dx"]
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    yp = forward(x[perm].contiguous(), w, b, d, P)
    dxp = backward(x[perm].contiguous(), g[perm].contiguous(), w, d, P, want=("dx",))["dx"]
    assert torch.equal(bits(yp), bits(y[perm])) and torch.equal(bits(dxp), bits(dx[perm]))
    for i in range(5):
        y1 = forward(x[i:i + 1].contiguous(), w, b, d, P)
        dx1 = backward(x[i:i + 1].contiguous(), g[i:i + 1].contiguous(), w, d, P, want=("dx",))["dx"]
        assert torch.equal(bits(y1[0]), bits(y[i])) and torch.equal(bits(dx1[0]), bits(dx[i])), i


@pytest.mark.parametrize("name", ["len00", "t128_k8d8", "fold9", "recipe_mdtc"])
def test_misaligned_bases_give_the_same_bits(name):
    """Row lengths that are multiples of four take the 16-byte accesses from aligned bases; a base 4 bytes off a 16-byte
    boundary takes the scalar ones: every result has the aligned run's bits."""
    c = dm.load_case(name)
    B, Cc, Tin, K, dd, P = dm.CASES[name][:6]
    assert Tin % 4 == 0 and dr.tout(Tin, K, dd, P) % 4 == 0
    d = dev(c)
    want = run_case(name)

    def shifted(t):
        _, v = guarded(t.shape, 1)
        v.copy_(t)
        return v

    xs, gs = shifted(d["x"]), shifted(d["g"])
    got = {"y": forward(xs, d["w"], d["bias"], c["d"], c["P"], offset=1)}
    got.update(backward(xs, gs, d["w"], c["d"], c["P"], offset=1))
    assert same(got, want)
    # only one tensor of a call off the boundary
    assert torch.equal(bits(forward(xs, d["w"], d["bias"], c["d"], c["P"])), bits(want["y"]))
    assert torch.equal(bits(forward(d["x"], d["w"], d["bias"], c["d"], c["P"], offset=1)), bits(want["y"]))
    assert same(backward(d["x"], gs, d["w"], c["d"], c["P"]), {k: want[k] for k in ("dx", "dw", "db")})
    assert same(backward(xs, d["g"], d["w"], c["d"], c["P"]), {k: want[k] for k in ("dx", "dw", "db")})


@pytest.mark.parametrize("name", ["p55_k8d8", "p1_k5d4", "len00", "t259_k8d8", "recipe_mdtc"])
def test_left_pad_is_an_explicitly_padded_input(name):
    """left_pad = P gives the bits of the same call on F.pad(x, (P, 0)) with left_pad = 0, dx cropped."""
    c = dm.load_case(name)
    d = dev(c)
    assert c["P"] > 0
    got = run_case(name)
    xp = F.pad(d["x"], (c["P"], 0), value=0.0).contiguous()
    ref = {"y": forward(xp, d["w"], d["bias"], c["d"], 0)}
    ref.update(backward(xp, d["g"], d["w"], c["d"], 0))
    ref["dx"] = ref["dx"][:, :, c["P"]:]
    assert same(got, ref)


def test_fp16_weights_miss_the_y_bar():
    """The negative control: the recipe case with its taps rounded to fp16 is outside the bar the float32 taps are held to."""
    c = dm.load_case("recipe_tcn")
    d = dev(c)
    y = forward(d["x"], d["w"].half().float(), d["bias"], c["d"], c["P"])
    u, bad = dm.units("recipe_tcn", {"y": y.cpu().numpy()})
    print(f"fp16 taps: y {u['y']:.1f} units (bar {dm.BARS['y']})")
    assert not bad and u["y"] > dm.BARS["y"]


def test_refused_calls_launch_nothing():
    lib = _capi.load()
    c = dm.load_case("g_small")
    d = dev(c)
    B, Cc, Tin, K, dd, P = dm.CASES["g_small"][:6]
    y = torch.full((B, Cc, dr.tout(Tin, K, dd, P)), CANARY, device="cuda")
    dx = torch.full_like(d["x"], CANARY)
    dw = torch.full_like(d["w"], CANARY)
    db = torch.full((Cc,), CANARY, device="cuda")
    nb = dr.workspace_bytes(B, Cc, Tin, K, dd, P)
    ws = torch.full((nb // 8 + 2,), CANARY, dtype=torch.float64, device="cuda")
    bias = torch.zeros(Cc, device="cuda")
    p = {k: v.data_ptr() for k, v in d.items() if v is not None}

    def fwd(x=p["x"], B=B, C=Cc, T=Tin, w=p["w"], b=bias.data_ptr(), K=K, d=dd, P=P, out=y.data_ptr()):
        return lib.wekws_hip_depthwise_conv1d_forward(x, B, C, T, w, b, K, d, P, out, _stream())

    def bwd(x=p["x"], g=p["g"], B=B, C=Cc, T=Tin, w=p["w"], K=K, d=dd, P=P, gx=dx.data_ptr(), gw=dw.data_ptr(), gb=db.data_ptr(),
            wsp=ws.data_ptr(), n=nb):
        return lib.wekws_hip_depthwise_conv1d_backward(x, g, B, C, T, w, K, d, P, gx, gw, gb, wsp, n, _stream())

    for kw in (dict(x=None), dict(w=None), dict(out=None), dict(B=0), dict(C=-1), dict(T=0), dict(K=0), dict(K=33), dict(d=0), dict(d=64),
               dict(P=-1), dict(P=17), dict(T=1, P=0)):
        assert fwd(**kw) == -1 and _capi.last_error() != "", kw
    for kw in (dict(x=None), dict(g=None), dict(w=None), dict(B=0), dict(C=0), dict(T=-2), dict(K=0), dict(K=33), dict(d=0), dict(d=64),
               dict(P=-1), dict(P=17), dict(T=1, P=0), dict(n=nb - 1), dict(wsp=None), dict(wsp=ws.data_ptr() + 8), dict(gx=None, wsp=None),
               dict(gw=None, n=0)):
        assert bwd(**kw) == -1 and _capi.last_error() != "", kw
    torch.cuda.synchronize()
    for t in (y, dx, dw, db, ws):
        assert bool((t == CANARY).all())
    assert fwd() == 0 and bwd() == 0                                             # and the same buffers are written by a good call
    torch.cuda.synchronize()
    for t in (y, dx, dw, db):
        assert not bool((t == CANARY).any())


def test_every_launch_beside_an_mfma_tenant(tenant):  # noqa: F811
    """The kernels on one stream, an MFMA-heavy forward on another: bit-identical to the solo run."""
    names = ["g_mid", "c9", "t259_k8d8", "fold15", "long", "recipe_tcn", "recipe_mdtc"]
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
