"""GPU: the dense Conv1d kernels (csrc/dense_conv.hip.h and the per-tap (B, C, T) fetch of csrc/linear_wgrad.hip.h) through
``wekws_amd.model.dense``: every case of tests/dense_conv_matrix.py against the float64 oracle at the bars and at the element
bounds; the device's bits against the emulation of the stated arithmetic; dw[:, :, k] and db against ``linear_weight_grad`` of the
shifted transposed copies, bit for bit; K = 1 against ``pointwise_conv1d``'s bits; the negative control; run-to-run and
stream-to-stream bits; the NaN and Inf properties; a row's independence of the other rows; refusals through the C ABI and the
wrapper; and a swapped CnnBlock in eval() with a carried cache."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dense_conv_matrix as dm
from wekws_amd import _capi
from wekws_amd.model import dense
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


def _run(name, x=None, w=None):
    """The case through the public op -> dict over quantities(name) of numpy arrays."""
    c = dm.load_case(name)
    s = c["spec"]
    off = s["flavour"] == "unaligned"
    xd = _dev(c["x"] if x is None else x, off).requires_grad_("dx" in s["wants"])
    wd = _dev(c["w"] if w is None else w, off).requires_grad_("dw" in s["wants"])
    bd = _dev(c["bias"]).requires_grad_("db" in s["wants"]) if c["bias"] is not None else None
    y = dense.dense_conv1d(xd, wd, bd, s["d"], s["P"])
    out = dict(y=y.detach().cpu().numpy())
    if not s["wants"]:
        return out
    y.backward(_dev(c["g"], off))
    for q, t in (("dx", xd), ("dw", wd), ("db", bd)):
        if q in s["wants"]:
            out[q] = t.grad.cpu().numpy()
        else:
            assert t is None or t.grad is None, (name, q)
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


@pytest.mark.parametrize("name", dm.case_names())
def test_cases_against_the_oracle(name, results, error_report):
    """Classes exactly, units under BARS, and every element inside the bounds of tests/dense_conv_matrix.py.
    Measured on MI355X: y at most 22.88 units (slices, K Ci = 2050; the recipe layers 14.95 .. 20.57), dx 8.82 (i65o65; the recipe
    layers 14.95 .. 18.57), dw 12.63 (rK-1; the recipe layers 5.95 .. 7.01), db 12.12 (i65o1; the recipe layers 5.08 .. 7.51); at most
    0.57 of an element bound."""
    got = results(name)
    assert list(got) == dm.quantities(name)
    u, bad = dm.units(name, got)
    excess = dm.element_excess(name, got)
    for q in got:
        print(f"{name}/{q}: {u[q]:.2f} units (bar {dm.BARS[q]:.0f}); element bound used {excess[q]:.3f}")
        error_report[f"dense_conv/{name}/{q}"] = u[q]
    assert not bad, (name, bad)
    for q in got:
        assert u[q] <= dm.BARS[q], (name, q, u[q], dm.BARS[q])
        assert excess[q] <= 1.0, (name, q, excess[q])


@pytest.mark.parametrize("name", dm.small_case_names())
def test_device_bits_are_the_stated_arithmetic(name, results):
    """The contract: the device's result is the emulation of tests/dense_conv_ref.py bit for bit -- float32 fmaf chains over the
    taps and, inside a tap, the channels, ascending from +0, the padding's zeros operands, and one bias addition; for dw and db
    chains of rows r = b Tout + t, slices and fold in double, one rounding.  NaNs are compared as NaNs, whatever their payload;
    zeros with their sign."""
    got, want = results(name), dm.emulated(name)
    for q in got:
        a, b = _bits(got[q]), _bits(want[q].reshape(got[q].shape))
        diff = int((a != b).sum())
        assert diff == 0, (name, q, f"{diff} of {a.size} elements differ", got[q].reshape(-1)[:4], want[q].reshape(-1)[:4])


@pytest.mark.parametrize("name", [n for n in dm.case_names() if dm.cases()[n]["wants"]])
def test_weight_gradients_are_linear_weight_grads_bits(name, results):
    """dw[:, :, k] and db are ``linear_weight_grad`` of the shifted, zero-padded, transposed contiguous copies, made here on the
    device, bit for bit: the per-tap fetch changes where the operands are read, never what is computed."""
    got, c = results(name), dm.load_case(name)
    assert "dw" in got or "db" in got
    s = c["spec"]
    xp = F.pad(_dev(c["x"]), (s["P"], 0))
    gt = _dev(c["g"]).transpose(1, 2).reshape(-1, s["Co"]).contiguous()
    for k in range(s["K"]):
        xt = xp[:, :, k * s["d"]:k * s["d"] + s["Tout"]].transpose(1, 2).reshape(-1, s["Ci"]).contiguous()
        dw, db = dl.linear_weight_grad(xt, gt, want_bias=True)
        if "dw" in got:
            assert np.array_equal(_bits(got["dw"][:, :, k]), _bits(dw.cpu().numpy())), (name, k)
        if "db" in got:
            assert np.array_equal(_bits(got["db"]), _bits(db.cpu().numpy())), name


def test_one_tap_is_the_pointwise_product_bit_for_bit(results):
    from wekws_amd.model import pointwise as pw
    c, got = dm.load_case("k1"), results("k1")
    xd, wd, bd = (_dev(c[k]).requires_grad_() for k in ("x", "w", "bias"))
    y = pw.pointwise_conv1d(xd, wd, bd)
    y.backward(_dev(c["g"]))
    for q, t in (("y", y.detach()), ("dx", xd.grad), ("dw", wd.grad), ("db", bd.grad)):
        assert np.array_equal(_bits(got[q]), _bits(t.cpu().numpy())), q


def test_negative_control_misses_the_bar(results):
    """w rounded to float16 at tcn_d4, on the device: what reduced-precision products would cost."""
    name = dm.CONTROL_CASE
    c = dm.load_case(name)
    got = _run(name, w=c["w"].astype(np.float16).astype(np.float32))
    u, bad = dm.units(name, dict(y=got["y"]))
    print(f"negative control: y {u['y']:.0f} units, bar {dm.BARS['y']:.0f}; the kernel itself {dm.units(name, results(name))[0]}")
    assert not bad and u["y"] >= 8 * dm.BARS["y"]
    assert abs(u["y"] - dm.CONTROL_UNITS) <= 0.05 * dm.CONTROL_UNITS


@pytest.mark.parametrize("name", ["k8d1p3", "slices", "tcn_d2"])
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


def test_a_nan_stays_in_its_window():
    """A NaN at x[b][i][n] makes exactly the y columns of row b whose window holds frame n, and dw[:, i, k] of the taps that
    reach it, NaN; every other element of y and dw, and dx and db, have the bits of the clean run.  A +Inf at g[b][o][t]: the
    classes of the oracle, exactly.  A +Inf weight over the padding, forward only: NaN there, as the reference."""
    c = dm.load_case("nan")
    s = c["spec"]
    frames, taps = dm.nan_hits(s)
    clean_x = c["x"].copy()
    clean_x[dm.NAN_B, dm.NAN_I, dm.nan_frame(s)] = 0.25
    got, clean = _run("nan"), _run("nan", x=clean_x)
    hit = np.zeros(got["y"].shape, bool)
    hit[dm.NAN_B, :, frames] = True
    assert np.isnan(got["y"][hit]).all() and all(np.isfinite(clean[q]).all() for q in clean)
    assert np.array_equal(got["y"][~hit].view(np.uint32), clean["y"][~hit].view(np.uint32))
    whit = np.zeros(got["dw"].shape, bool)
    whit[:, dm.NAN_I, taps] = True
    assert np.isnan(got["dw"][whit]).all()
    assert np.array_equal(got["dw"][~whit].view(np.uint32), clean["dw"][~whit].view(np.uint32))
    assert np.array_equal(got["dx"].view(np.uint32), clean["dx"].view(np.uint32))
    assert np.array_equal(got["db"].view(np.uint32), clean["db"].view(np.uint32))
    inf, ref = _run("inf"), dm.oracle("inf")
    assert all(dm.same_classes(inf[q], ref[q]) for q in inf)
    assert np.isinf(inf["dw"][dm.INF_O]).any() and inf["db"][dm.INF_O] == np.inf
    winf, s = _run("winf"), dm.cases()["winf"]
    assert list(winf) == ["y"] and dm.same_classes(winf["y"], dm.oracle("winf")["y"])
    assert np.isnan(winf["y"][:, dm.WINF_O, :s["P"]]).all() and np.isinf(winf["y"][:, dm.WINF_O, s["P"]:]).all()


def test_a_rows_results_do_not_depend_on_the_other_rows(results):
    """y[b] and dx[b] of the case equal those of row b run alone, and stay when every other row changes, bit for bit."""
    name = "k8d1p3"
    c, got = dm.load_case(name), results(name)
    s = c["spec"]
    w, bias = _dev(c["w"]), _dev(c["bias"])
    for b in range(s["B"]):
        x = _dev(c["x"][b:b + 1]).requires_grad_()
        y = dense.dense_conv1d(x, w, bias, s["d"], s["P"])
        y.backward(_dev(c["g"][b:b + 1]))
        assert np.array_equal(_bits(y.detach().cpu().numpy()), _bits(got["y"][b:b + 1])), b
        assert np.array_equal(_bits(x.grad.cpu().numpy()), _bits(got["dx"][b:b + 1])), b
    other = c["x"].copy()
    other[0] = np.nan
    x = _dev(other).requires_grad_()
    g = c["g"].copy()
    g[0] = np.inf
    y = dense.dense_conv1d(x, w, bias, s["d"], s["P"])
    y.backward(_dev(g))
    assert np.array_equal(_bits(y.detach().cpu().numpy()[1:]), _bits(got["y"][1:]))
    assert np.array_equal(_bits(x.grad.cpu().numpy()[1:]), _bits(got["dx"][1:]))


def test_refusals_leave_the_outputs_untouched():
    lib = _capi.load()
    B, Ci, Tin, Co, K, d, P = 2, 20, 9, 16, 3, 2, 3
    Tout = Tin + P - (K - 1) * d
    x, g, w, b = (torch.randn(B, Ci, Tin, device="cuda"), torch.randn(B, Co, Tout, device="cuda"), torch.randn(Co, Ci, K, device="cuda"),
                  torch.randn(Co, device="cuda"))
    nbytes = lib.wekws_hip_dense_conv1d_workspace_bytes(B, Ci, Tin, Co, K, d, P)
    ws = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device="cuda")
    y, dx = torch.full((B, Co, Tout), 1.5, device="cuda"), torch.full((B, Ci, Tin), -2.5, device="cuda")
    dw, db = torch.full((Co, Ci, K), 7.5, device="cuda"), torch.full((Co,), -3.25, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    forward = {
        "B < 1": (p(x), 0, Ci, Tin, p(w), p(b), Co, K, d, P, p(y)),
        "Ci too large": (p(x), B, 65536, Tin, p(w), p(b), Co, K, d, P, p(y)),
        "Tin < 1": (p(x), B, Ci, 0, p(w), p(b), Co, K, d, P, p(y)),
        "Co = 0": (p(x), B, Ci, Tin, p(w), p(b), 0, K, d, P, p(y)),
        "K = 33": (p(x), B, Ci, Tin, p(w), p(b), Co, 33, 1, 0, p(y)),
        "d = 0": (p(x), B, Ci, Tin, p(w), p(b), Co, K, 0, 0, p(y)),
        "window": (p(x), B, Ci, Tin, p(w), p(b), Co, 2, 256, 256, p(y)),
        "left_pad too large": (p(x), B, Ci, Tin, p(w), p(b), Co, K, d, 5, p(y)),
        "left_pad < 0": (p(x), B, Ci, Tin, p(w), p(b), Co, K, d, -1, p(y)),
        "no output frame": (p(x), B, Ci, 4, p(w), p(b), Co, K, d, 0, p(y)),
        "grid": (p(x), 2 ** 31 - 1, Ci, 65, p(w), p(b), Co, 2, 1, 1, p(y)),
        "x NULL": (None, B, Ci, Tin, p(w), p(b), Co, K, d, P, p(y)),
        "w NULL": (p(x), B, Ci, Tin, None, p(b), Co, K, d, P, p(y)),
        "y NULL": (p(x), B, Ci, Tin, p(w), p(b), Co, K, d, P, None),
    }
    for what, args in forward.items():
        assert lib.wekws_hip_dense_conv1d_forward(*args, stream) == -1, what          # WEKWS_HIP_EINVAL
    outs = (p(dx), p(dw), p(db))
    backward = {
        "B < 1": (p(x), p(g), 0, Ci, Tin, p(w), Co, K, d, P, *outs, p(ws), nbytes),
        "Ci too large": (p(x), p(g), B, 65536, Tin, p(w), Co, K, d, P, *outs, p(ws), nbytes),
        "K = 0": (p(x), p(g), B, Ci, Tin, p(w), Co, 0, d, 0, *outs, p(ws), nbytes),
        "left_pad too large": (p(x), p(g), B, Ci, Tin, p(w), Co, K, d, 5, *outs, p(ws), nbytes),
        "no output": (p(x), p(g), B, Ci, Tin, p(w), Co, K, d, P, None, None, None, p(ws), nbytes),
        "x NULL": (None, p(g), B, Ci, Tin, p(w), Co, K, d, P, *outs, p(ws), nbytes),
        "grad_y NULL": (p(x), None, B, Ci, Tin, p(w), Co, K, d, P, *outs, p(ws), nbytes),
        "w NULL": (p(x), p(g), B, Ci, Tin, None, Co, K, d, P, *outs, p(ws), nbytes),
        "workspace NULL": (p(x), p(g), B, Ci, Tin, p(w), Co, K, d, P, *outs, None, nbytes),
        "workspace unaligned": (p(x), p(g), B, Ci, Tin, p(w), Co, K, d, P, *outs, p(ws) + 8, nbytes),
        "workspace small": (p(x), p(g), B, Ci, Tin, p(w), Co, K, d, P, *outs, p(ws), nbytes - 16),
    }
    for what, args in backward.items():
        assert lib.wekws_hip_dense_conv1d_backward(*args, stream) == -1, what
    torch.cuda.synchronize()
    assert bool((y == 1.5).all()) and bool((dx == -2.5).all()) and bool((dw == 7.5).all()) and bool((db == -3.25).all())
    # the accepted calls write every element; grad_x alone needs no workspace
    assert lib.wekws_hip_dense_conv1d_forward(p(x), B, Ci, Tin, p(w), p(b), Co, K, d, P, p(y), stream) == 0
    assert lib.wekws_hip_dense_conv1d_backward(p(x), p(g), B, Ci, Tin, p(w), Co, K, d, P, p(dx), None, None, None, 0, stream) == 0
    assert lib.wekws_hip_dense_conv1d_backward(p(x), p(g), B, Ci, Tin, p(w), Co, K, d, P, None, p(dw), p(db), p(ws), nbytes, stream) == 0
    x64, g64, w64 = (t.double().requires_grad_() for t in (x, g, w))
    b64 = b.double().requires_grad_()
    want = F.conv1d(F.pad(x64, (P, 0)), w64, b64, dilation=d)
    want.backward(g64.detach())
    want = want.detach()
    assert float((y - want).abs().max()) <= 1e-4 and float((dx - x64.grad).abs().max()) <= 1e-4
    assert float((dw - w64.grad).abs().max()) <= 1e-4 and float((db - b64.grad).abs().max()) <= 1e-4
    for bad in (lambda: dense.dense_conv1d(x.cpu(), w.cpu()), lambda: dense.dense_conv1d(x, w[:, :-1]),
                lambda: dense.dense_conv1d(x.double(), w.double()), lambda: dense.dense_conv1d(x, w, b[:-1]),
                lambda: dense.dense_conv1d(x, w, b, d, 5), lambda: dense.dense_conv1d(x, w, b, d, -1),
                lambda: dense.dense_conv1d(x, w, b, 0, 0), lambda: dense.dense_conv1d(x, w, b, 128, 0),
                lambda: dense.dense_conv1d(x[:, :, :4], w, b, d, 0), lambda: dense.dense_conv1d(x[0], w, b)):
        with pytest.raises(ValueError):
            bad()


def test_a_swapped_cnn_block_in_eval_with_a_carried_cache():
    """A CnnBlock with its dense convolution swapped, in eval() under no_grad: one shot and in two chunks with the carried cache,
    against the unswapped block within the y bar, with the unswapped block's caches bit for bit; the swapped convolution on a
    slice of the frames equal to the slice of its result bit for bit."""
    from wekws_amd.model import tcn
    torch.manual_seed(21)
    ref = tcn.CnnBlock(24, 5, 2, 0.0).cuda().eval()
    dev = tcn.CnnBlock(24, 5, 2, 0.0).cuda().eval()
    dev.load_state_dict(ref.state_dict())
    assert dense.use_device_dense_convs(dev) == 1 and type(dev.cnn[0]) is dense.DenseConv1d
    x = torch.randn(3, 24, 41, device="cuda")
    empty = torch.zeros(0, 0, 0, device="cuda")
    with torch.no_grad():
        want, wcache = ref(x, empty)
        got, cache = dev(x, empty)
        y1, c1 = dev(x[:, :, :17].contiguous(), empty)
        y2, c2 = dev(x[:, :, 17:].contiguous(), c1)
        r1, rc1 = ref(x[:, :, :17].contiguous(), empty)
    assert not got.requires_grad and torch.equal(cache, wcache) and torch.equal(c2, cache) and torch.equal(c1, rc1)
    assert dm.tensor_units(got.cpu().numpy(), want.double().cpu().numpy()) <= dm.BARS["y"]
    assert dm.tensor_units(torch.cat([y1, y2], 2).cpu().numpy(), want.double().cpu().numpy()) <= dm.BARS["y"]
    with torch.no_grad():
        whole = dev.cnn[0](x, 8)
        assert whole.shape == x.shape
        tail = dev.cnn[0](x[:, :, 9:].contiguous(), 0)                       # frames 17 .. 40: their windows start at frame 9
        assert torch.equal(tail, whole[:, :, 17:])
        assert torch.equal(dev.cnn[0](x[1:2].contiguous(), 8), whole[1:2])
