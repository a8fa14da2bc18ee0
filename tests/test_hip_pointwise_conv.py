"""GPU: the pointwise Conv1d kernels (csrc/pointwise_conv.hip.h and the (B, C, T) fetch of csrc/linear_wgrad.hip.h) through
``wekws_amd.model.pointwise``: every case of tests/pointwise_conv_matrix.py against the float64 oracle at the bars and at the
element bounds; the device's bits against the emulation of the stated arithmetic; dw and db against ``linear_weight_grad`` of the
transposed copies, bit for bit; the negative control; run-to-run and stream-to-stream bits; the NaN properties; refusals through
the C ABI; and PointwiseConv1d inside a TCNBlock in eval() with a carried cache."""
import ctypes

import numpy as np
import pytest
import torch

from tests import pointwise_conv_matrix as pm
from wekws_amd import _capi
from wekws_amd.model import linear as dl
from wekws_amd.model import pointwise as pw

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
    c = pm.load_case(name)
    s = c["spec"]
    off = s["flavour"] == "unaligned"
    xd = _dev(c["x"] if x is None else x, off).requires_grad_("dx" in s["wants"])
    wd = _dev((c["w"] if w is None else w)[:, :, None], off).requires_grad_("dw" in s["wants"])
    bd = _dev(c["bias"]).requires_grad_("db" in s["wants"]) if c["bias"] is not None else None
    y = pw.pointwise_conv1d(xd, wd, bd)
    y.backward(_dev(c["g"], off))
    out = dict(y=y.detach().cpu().numpy())
    for q, t in (("dx", xd), ("dw", wd), ("db", bd)):
        if q in s["wants"]:
            out[q] = t.grad.cpu().numpy().reshape(pm.oracle(name)[q].shape)
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


@pytest.mark.parametrize("name", pm.case_names())
def test_cases_against_the_oracle(name, results, error_report):
    """Classes exactly, units under BARS, and every element inside the bounds of tests/pointwise_conv_matrix.py.
    Measured on MI355X: y at most 23.35 units (slices, Ci = 2049; the recipe shapes 4.11 .. 11.85), dx 13.22 (ds256), dw 12.93
    (large; the recipe shapes 5.44 .. 6.53), db 13.06 (straddle; the recipe shapes 7.10 .. 9.17); at most 0.52 of an element bound."""
    got = results(name)
    assert list(got) == pm.quantities(name)
    u, bad = pm.units(name, got)
    excess = pm.element_excess(name, got)
    for q in got:
        print(f"{name}/{q}: {u[q]:.2f} units (bar {pm.BARS[q]:.0f}); element bound used {excess[q]:.3f}")
        error_report[f"pointwise_conv/{name}/{q}"] = u[q]
    assert not bad, (name, bad)
    for q in got:
        assert u[q] <= pm.BARS[q], (name, q, u[q], pm.BARS[q])
        assert excess[q] <= 1.0, (name, q, excess[q])


@pytest.mark.parametrize("name", pm.small_case_names())
def test_device_bits_are_the_stated_arithmetic(name, results):
    """The contract: the device's result is the emulation of tests/pointwise_conv_ref.py bit for bit -- float32 fmaf chains over
    the channels ascending from +0 and one bias addition; for dw and db chains of K rows r = b T + t, slices and fold in double,
    one rounding.  NaNs are compared as NaNs, whatever their payload; zeros with their sign."""
    got, want = results(name), pm.emulated(name)
    for q in got:
        a, b = _bits(got[q]), _bits(want[q].reshape(got[q].shape))
        diff = int((a != b).sum())
        assert diff == 0, (name, q, f"{diff} of {a.size} elements differ", got[q].reshape(-1)[:4], want[q].reshape(-1)[:4])


@pytest.mark.parametrize("name", pm.case_names())
def test_weight_gradients_are_linear_weight_grads_bits(name, results):
    """dw and db are ``linear_weight_grad`` of the transposed contiguous copies, made here on the device, bit for bit: the
    (B, C, T) fetch changes where the operands are read, never what is computed."""
    got, c = results(name), pm.load_case(name)
    assert "dw" in got or "db" in got
    s = c["spec"]
    xt = _dev(c["x"]).transpose(1, 2).reshape(-1, s["Ci"]).contiguous()
    gt = _dev(c["g"]).transpose(1, 2).reshape(-1, s["Co"]).contiguous()
    dw, db = dl.linear_weight_grad(xt, gt, want_bias=True)
    if "dw" in got:
        assert np.array_equal(_bits(got["dw"]), _bits(dw.cpu().numpy())), name
    if "db" in got:
        assert np.array_equal(_bits(got["db"]), _bits(db.cpu().numpy())), name


def test_negative_control_misses_the_bar(results):
    """w rounded to float16 at ds_tcn, on the device: what reduced-precision products would cost."""
    name = pm.CONTROL_CASE
    c = pm.load_case(name)
    got = _run(name, w=c["w"].astype(np.float16).astype(np.float32))
    u, bad = pm.units(name, dict(y=got["y"]))
    print(f"negative control: y {u['y']:.0f} units, bar {pm.BARS['y']:.0f}; the kernel itself {pm.units(name, results(name))[0]}")
    assert not bad and u["y"] >= 8 * pm.BARS["y"]
    assert abs(u["y"] - pm.CONTROL_UNITS) <= 0.05 * pm.CONTROL_UNITS


@pytest.mark.parametrize("name", ["ragged", "slices", "mdtc_pre"])
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
    """A NaN at x[b][i][t] makes y[b][:, t] and column i of dw NaN; every other element of y and dw, and dx and db, have the bits
    of the clean run.  A +Inf at g[b][o][t]: the classes of the oracle, exactly."""
    c = pm.load_case("nan")
    clean_x = c["x"].copy()
    clean_x[pm.NAN_B, pm.NAN_I, pm.NAN_T] = 0.25
    got, clean = results("nan"), _run("nan", x=clean_x)
    hit = np.zeros(got["y"].shape, bool)
    hit[pm.NAN_B, :, pm.NAN_T] = True
    assert np.isnan(got["y"][hit]).all() and all(np.isfinite(clean[q]).all() for q in clean)
    assert np.array_equal(got["y"][~hit].view(np.uint32), clean["y"][~hit].view(np.uint32))
    cols = [i for i in range(got["dw"].shape[1]) if i != pm.NAN_I]
    assert np.isnan(got["dw"][:, pm.NAN_I]).all()
    assert np.array_equal(got["dw"][:, cols].view(np.uint32), clean["dw"][:, cols].view(np.uint32))
    assert np.array_equal(got["dx"].view(np.uint32), clean["dx"].view(np.uint32))
    assert np.array_equal(got["db"].view(np.uint32), clean["db"].view(np.uint32))
    inf, ref = results("inf"), pm.oracle("inf")
    assert all(pm.same_classes(inf[q], ref[q]) for q in inf)
    assert np.isinf(inf["dx"][pm.INF_B, :, pm.INF_T]).all() and np.isinf(inf["dw"][pm.INF_O]).all() and inf["db"][pm.INF_O] == np.inf


def test_refusals_leave_the_outputs_untouched():
    lib = _capi.load()
    B, Ci, T, Co = 2, 20, 9, 16
    x, g, w, b = (torch.randn(B, Ci, T, device="cuda"), torch.randn(B, Co, T, device="cuda"), torch.randn(Co, Ci, device="cuda"),
                  torch.randn(Co, device="cuda"))
    nbytes = lib.wekws_hip_pointwise_conv1d_workspace_bytes(B, Ci, T, Co)
    ws = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device="cuda")
    y, dx = torch.full((B, Co, T), 1.5, device="cuda"), torch.full((B, Ci, T), -2.5, device="cuda")
    dw, db = torch.full((Co, Ci), 7.5, device="cuda"), torch.full((Co,), -3.25, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    forward = {
        "B < 1": (p(x), 0, Ci, T, p(w), p(b), Co, p(y)),
        "Ci = 0": (p(x), B, 0, T, p(w), p(b), Co, p(y)),
        "Ci too large": (p(x), B, 65536, T, p(w), p(b), Co, p(y)),
        "T < 1": (p(x), B, Ci, 0, p(w), p(b), Co, p(y)),
        "Co = 0": (p(x), B, Ci, T, p(w), p(b), 0, p(y)),
        "Co too large": (p(x), B, Ci, T, p(w), p(b), 65536, p(y)),
        "grid": (p(x), 2 ** 31 - 1, Ci, 65, p(w), p(b), Co, p(y)),
        "x NULL": (None, B, Ci, T, p(w), p(b), Co, p(y)),
        "w NULL": (p(x), B, Ci, T, None, p(b), Co, p(y)),
        "y NULL": (p(x), B, Ci, T, p(w), p(b), Co, None),
    }
    for what, args in forward.items():
        assert lib.wekws_hip_pointwise_conv1d_forward(*args, stream) == -1, what          # WEKWS_HIP_EINVAL
    outs = (p(dx), p(dw), p(db))
    backward = {
        "B < 1": (p(x), p(g), 0, Ci, T, p(w), Co, *outs, p(ws), nbytes),
        "Ci too large": (p(x), p(g), B, 65536, T, p(w), Co, *outs, p(ws), nbytes),
        "T < 1": (p(x), p(g), B, Ci, 0, p(w), Co, *outs, p(ws), nbytes),
        "Co = 0": (p(x), p(g), B, Ci, T, p(w), 0, *outs, p(ws), nbytes),
        "no output": (p(x), p(g), B, Ci, T, p(w), Co, None, None, None, p(ws), nbytes),
        "x NULL": (None, p(g), B, Ci, T, p(w), Co, *outs, p(ws), nbytes),
        "grad_y NULL": (p(x), None, B, Ci, T, p(w), Co, *outs, p(ws), nbytes),
        "w NULL": (p(x), p(g), B, Ci, T, None, Co, *outs, p(ws), nbytes),
        "workspace NULL": (p(x), p(g), B, Ci, T, p(w), Co, *outs, None, nbytes),
        "workspace unaligned": (p(x), p(g), B, Ci, T, p(w), Co, *outs, p(ws) + 8, nbytes),
        "workspace small": (p(x), p(g), B, Ci, T, p(w), Co, *outs, p(ws), nbytes - 16),
    }
    for what, args in backward.items():
        assert lib.wekws_hip_pointwise_conv1d_backward(*args, stream) == -1, what
    torch.cuda.synchronize()
    assert bool((y == 1.5).all()) and bool((dx == -2.5).all()) and bool((dw == 7.5).all()) and bool((db == -3.25).all())
    # the accepted calls write every element; grad_x alone needs no workspace
    assert lib.wekws_hip_pointwise_conv1d_forward(p(x), B, Ci, T, p(w), p(b), Co, p(y), stream) == 0
    assert lib.wekws_hip_pointwise_conv1d_backward(p(x), p(g), B, Ci, T, p(w), Co, p(dx), None, None, None, 0, stream) == 0
    assert lib.wekws_hip_pointwise_conv1d_backward(p(x), p(g), B, Ci, T, p(w), Co, None, p(dw), p(db), p(ws), nbytes, stream) == 0
    x64, g64, w64 = x.double(), g.double(), w.double()
    assert float((y - (torch.matmul(w64, x64) + b.double()[None, :, None])).abs().max()) <= 1e-4
    assert float((dx - torch.matmul(w64.t(), g64)).abs().max()) <= 1e-4
    assert float((dw - torch.einsum("bot,bit->oi", g64, x64)).abs().max()) <= 1e-4
    assert float((db - g64.sum((0, 2))).abs().max()) <= 1e-4
    with pytest.raises(ValueError):
        pw.pointwise_conv1d(x.cpu(), w.cpu()[:, :, None])
    with pytest.raises(ValueError):
        pw.pointwise_conv1d(x, w[:, :-1, None])
    with pytest.raises(ValueError):
        pw.pointwise_conv1d(x.double(), w.double()[:, :, None])


def test_pointwise_conv1d_in_a_tcn_block_in_eval_with_a_carried_cache():
    """A TCNBlock with its two pointwise convolutions swapped, in eval() under no_grad: one shot and in two chunks with the
    carried cache, against the unswapped block within the y bar; and the swapped convolution alone on a slice of the frames
    equal to the slice of its result bit for bit (a frame's result depends on its column alone)."""
    from wekws_amd.model import mdtc
    torch.manual_seed(21)
    ref = mdtc.TCNBlock(24, 24, 5, 2, True).cuda().eval()
    dev = mdtc.TCNBlock(24, 24, 5, 2, True).cuda().eval()
    dev.load_state_dict(ref.state_dict())
    assert pw.use_device_pointwise_convs(dev) == 2
    x = torch.randn(3, 24, 41, device="cuda")
    with torch.no_grad():
        want, wcache = ref(x, torch.zeros(0, 0, 0, device="cuda"))
        got, cache = dev(x, torch.zeros(0, 0, 0, device="cuda"))
        y1, c1 = dev(x[:, :, :17].contiguous(), torch.zeros(0, 0, 0, device="cuda"))
        y2, c2 = dev(x[:, :, 17:].contiguous(), c1)
    assert not got.requires_grad and torch.equal(cache, wcache) and torch.equal(c2, cache)
    assert pm.tensor_units(got.cpu().numpy(), want.double().cpu().numpy()) <= pm.BARS["y"]
    assert pm.tensor_units(torch.cat([y1, y2], 2).cpu().numpy(), want.double().cpu().numpy()) <= pm.BARS["y"]
    with torch.no_grad():
        whole = dev.conv2(x)
        assert torch.equal(dev.conv2(x[:, :, 17:].contiguous()), whole[:, :, 17:])
        assert torch.equal(dev.conv2(x[1:2, :, 5:6].contiguous()), whole[1:2, :, 5:6])
