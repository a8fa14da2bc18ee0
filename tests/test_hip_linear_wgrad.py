"""GPU: the Linear weight-gradient kernels (csrc/linear_wgrad.hip.h) through ``wekws_amd.model.linear``: every case of
tests/linear_wgrad_matrix.py against the float64 oracle at the bars and at the element bound; the device's bits against the
emulation of the stated arithmetic; the negative control; run-to-run and stream-to-stream bits; the NaN properties; refusals
through the C ABI; and DeviceLinear's forward and input gradient against nn.Linear's, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import linear_wgrad_matrix as lm
from wekws_amd import _capi
from wekws_amd.model import linear as dl

pytestmark = pytest.mark.gpu


def _dev(a, offset=False):
    """A device copy; ``offset``: at a base 4 bytes past a 16-byte boundary."""
    t = torch.from_numpy(np.array(a, copy=True, order="C"))
    if not offset:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _run(name, x=None):
    """The case through the public ops -> dict over quantities(name) of numpy arrays."""
    c = lm.load_case(name)
    s = c["spec"]
    off = s["flavour"] == "unaligned"
    xd, gd = _dev(c["x"] if x is None else x, off), _dev(c["g"], off)
    out = {}
    if s["weight"]:
        dw, db = dl.linear_weight_grad(xd, gd, want_bias=s["bias"])
        assert (db is None) == (not s["bias"])
        out["dw"] = dw.cpu().numpy()
        if db is not None:
            out["db"] = db.cpu().numpy()
    else:                                                   # dw not wanted: autograd asks linear() for the bias gradient alone
        w = torch.zeros(s["O"], s["I"], device="cuda")
        b = torch.zeros(s["O"], device="cuda", requires_grad=True)
        dl.linear(xd, w, b).backward(gd)
        assert w.grad is None
        out["db"] = b.grad.cpu().numpy()
    return out


@pytest.fixture(scope="module")
def results():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(name)
        return cache[name]
    return get


def _bits(a):
    """float32 bits with every NaN made one NaN: payloads are not part of the contract."""
    a = np.ascontiguousarray(a, np.float32).copy()
    a[np.isnan(a)] = np.float32(np.nan)
    return a.view(np.uint32)


@pytest.mark.parametrize("name", lm.case_names())
def test_cases_against_the_oracle(name, results, error_report):
    """Classes exactly, units under BARS, and every element inside U |ref| + gamma(K) sum |g x| (tests/linear_wgrad_matrix.py).
    Measured on MI355X: dw at most 13.78 units (rK; the recipe shapes 7.43 .. 9.59), db at most 10.88 (rK+1; the recipe shapes
    6.25 .. 10.55); at most 0.008 of the element bound."""
    got = results(name)
    assert list(got) == lm.quantities(name)
    u, bad = lm.units(name, got)
    excess = lm.element_excess(name, got)
    for q in got:
        print(f"{name}/{q}: {u[q]:.2f} units (bar {lm.BARS[q]:.0f}); element bound used {excess[q]:.3f}")
        error_report[f"linear_wgrad/{name}/{q}"] = u[q]
    assert not bad, (name, bad)
    for q in got:
        assert u[q] <= lm.BARS[q], (name, q, u[q], lm.BARS[q])
        assert excess[q] <= 1.0, (name, q, excess[q])


@pytest.mark.parametrize("name", lm.small_case_names())
def test_device_bits_are_the_stated_arithmetic(name, results):
    """The contract: the device's result is tests/linear_wgrad_ref.py::emulate bit for bit -- chains of K rows in float32 fmaf,
    slices and fold in double, one rounding.  NaNs are compared as NaNs, whatever their payload; zeros with their sign."""
    got, want = results(name), lm.emulated(name)
    for q in got:
        a, b = _bits(got[q]), _bits(want[q].reshape(got[q].shape))
        diff = int((a != b).sum())
        assert diff == 0, (name, q, f"{diff} of {a.size} elements differ", got[q].reshape(-1)[:4], want[q].reshape(-1)[:4])


def test_negative_control_misses_the_bar(results):
    """x rounded to float16 at gru_ih, on the device: what reduced-precision products would cost."""
    c = lm.load_case("gru_ih")
    got = _run("gru_ih", x=c["x"].astype(np.float16).astype(np.float32))
    u, bad = lm.units("gru_ih", dict(dw=got["dw"]))
    print(f"negative control: dw {u['dw']:.0f} units, bar {lm.BARS['dw']:.0f}; the kernel itself {lm.units('gru_ih', results('gru_ih'))[0]}")
    assert not bad and u["dw"] >= 8 * lm.BARS["dw"]
    assert abs(u["dw"] - lm.CONTROL_UNITS) <= 0.05 * lm.CONTROL_UNITS


@pytest.mark.parametrize("name", ["odd", "slices", "fsmn_in"])
def test_two_runs_and_a_second_stream_give_the_same_bits(name, results):
    first = results(name)
    again = _run(name)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _run(name)
    side.synchronize()
    for q in first:
        assert np.array_equal(_bits(first[q]), _bits(again[q])), (name, q)
        assert np.array_equal(_bits(first[q]), _bits(other[q])), (name, q)


def test_a_nan_stays_in_its_column(results):
    """A NaN at x[r][i] makes column i of dw NaN; every other column and db have the bits of the clean run.  A +Inf at g[r][o]:
    the classes of the oracle, exactly (row o of dw is +-Inf by the sign of x[r][i], db[o] is +Inf)."""
    c = lm.load_case("nan")
    clean_x = c["x"].copy()
    clean_x[lm.NAN_R, lm.NAN_I] = 0.25
    got, clean = results("nan"), _run("nan", x=clean_x)
    cols = [i for i in range(got["dw"].shape[1]) if i != lm.NAN_I]
    assert np.isnan(got["dw"][:, lm.NAN_I]).all() and np.isfinite(clean["dw"]).all()
    assert np.array_equal(got["dw"][:, cols].view(np.uint32), clean["dw"][:, cols].view(np.uint32))
    assert np.array_equal(got["db"].view(np.uint32), clean["db"].view(np.uint32))
    inf, ref = results("inf"), lm.oracle("inf")
    assert lm.same_classes(inf["dw"], ref["dw"]) and lm.same_classes(inf["db"], ref["db"])
    assert np.isinf(inf["dw"][lm.INF_O]).all() and inf["db"][lm.INF_O] == np.inf


def test_refusals_leave_the_outputs_untouched():
    lib = _capi.load()
    R, O, I = 40, 16, 20
    x, g = torch.randn(R, I, device="cuda"), torch.randn(R, O, device="cuda")
    nbytes = lib.wekws_hip_linear_wgrad_workspace_bytes(R, O, I)
    ws = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device="cuda")
    dw, db = torch.full((O, I), 7.5, device="cuda"), torch.full((O,), -3.25, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    calls = {
        "R < 1": (p(x), p(g), 0, O, I, p(dw), p(db), p(ws), nbytes),
        "O = 0": (p(x), p(g), R, 0, I, p(dw), p(db), p(ws), nbytes),
        "O too large": (p(x), p(g), R, 65536, I, p(dw), p(db), p(ws), nbytes),
        "I = 0": (p(x), p(g), R, O, 0, p(dw), p(db), p(ws), nbytes),
        "I too large": (p(x), p(g), R, O, 65536, p(dw), p(db), p(ws), nbytes),
        "no output": (p(x), p(g), R, O, I, None, None, p(ws), nbytes),
        "x NULL": (None, p(g), R, O, I, p(dw), p(db), p(ws), nbytes),
        "g NULL": (p(x), None, R, O, I, p(dw), p(db), p(ws), nbytes),
        "workspace NULL": (p(x), p(g), R, O, I, p(dw), p(db), None, nbytes),
        "workspace unaligned": (p(x), p(g), R, O, I, p(dw), p(db), p(ws) + 8, nbytes),
        "workspace small": (p(x), p(g), R, O, I, p(dw), p(db), p(ws), nbytes - 16),
    }
    for what, args in calls.items():
        assert lib.wekws_hip_linear_wgrad(*args, stream) == -1, what            # WEKWS_HIP_EINVAL
    torch.cuda.synchronize()
    assert bool((dw == 7.5).all()) and bool((db == -3.25).all())
    # and the accepted call writes every element of both
    assert lib.wekws_hip_linear_wgrad(p(x), p(g), R, O, I, p(dw), p(db), p(ws), nbytes, stream) == 0
    ref_w, ref_b = g.double().t().mm(x.double()), g.double().sum(0)
    assert float((dw - ref_w).abs().max()) <= 1e-4 and float((db - ref_b).abs().max()) <= 1e-4
    with pytest.raises(ValueError):
        dl.linear_weight_grad(x.cpu(), g.cpu())
    with pytest.raises(ValueError):
        dl.linear_weight_grad(x, g[:-1])
    with pytest.raises(ValueError):
        dl.linear_weight_grad(x.double(), g.double())


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", [(7, 20), (3, 5, 20)])
def test_device_linear_forward_and_dx_are_torchs_bits(bias, shape):
    torch.manual_seed(13)
    ref = nn.Linear(20, 24, bias=bias).cuda()
    dev = dl.DeviceLinear.sharing(ref)
    assert dev.weight is ref.weight and dev.bias is ref.bias
    x = torch.randn(*shape, device="cuda")
    sel = torch.randn(*shape[:-1], 24, device="cuda")
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya = ref(xa)
    (ya * sel).sum().backward()
    gw = ref.weight.grad.clone()
    gb = ref.bias.grad.clone() if bias else None
    ref.zero_grad()
    yb = dev(xb)
    (yb * sel).sum().backward()
    assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    # the parameter gradients are the kernel's: against float64, in units of 2^-24 of the tensor's max, at the bars
    w64 = sel.double().reshape(-1, 24).t().mm(x.double().reshape(-1, 20))
    assert lm.tensor_units(dev.weight.grad.cpu().numpy(), w64.cpu().numpy()) <= lm.BARS["dw"]
    assert lm.tensor_units(gw.cpu().numpy(), w64.cpu().numpy()) <= lm.BARS["dw"]
    if bias:
        b64 = sel.double().reshape(-1, 24).sum(0)
        assert lm.tensor_units(dev.bias.grad.cpu().numpy(), b64.cpu().numpy()) <= lm.BARS["db"]
        assert gb is not None
    # no gradient wanted for the parameters: none is computed
    frozen = dl.DeviceLinear(20, 24, bias=bias).cuda().requires_grad_(False)
    xc = x.clone().requires_grad_()
    frozen(xc).sum().backward()
    assert frozen.weight.grad is None and xc.grad is not None
