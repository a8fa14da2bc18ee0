"""GPU: wekws_amd.model.gru -- every case of tests/gru_train_matrix.py through ``DeviceGRU`` against the float64 oracle at the
bars, the negative control, row independence and reproducibility of ``gru_scan`` bit for bit, refusals through the C ABI that
write nothing, and the modules that take torch's own path."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import gru_train_matrix as gm
from wekws_amd import _capi
from wekws_amd.model import gru as dg

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.mark.parametrize("name", gm.case_names())
def test_device_gru_against_the_oracle(name, error_report):
    m = gm.module(name, dg.DeviceGRU, device="cuda")
    got = gm.run_module(name, m, device="cuda")
    u, bad = gm.units(name, got)
    print(f"{name}: device units {({k: round(v, 2) for k, v in u.items()})}")
    for q, v in u.items():
        error_report[f"gru_train/{name}/{q}"] = v
    assert not bad, (name, bad)
    assert all(u[q] <= gm.BARS[q] for q in u), (name, u)


def test_negative_control_misses_its_bar():
    """W_hh rounded to float16 at the recipe case: the bar of y catches what reduced-precision products would cost."""
    m = gm.module("recipe", dg.DeviceGRU, device="cuda", w_hh_dtype=torch.float16)
    c = gm.load_case("recipe")
    with torch.no_grad():
        y, _ = m(torch.from_numpy(c["x"].copy()).cuda())
    u = gm.tensor_units(y.cpu().numpy(), gm.oracle("recipe")["y"][0])
    print(f"negative control: {u:.0f} units, bar {gm.BARS['y']}")
    assert u > gm.BARS["y"]


def _scan(gi, w, b, h0, gy, ghn):
    """gru_scan forward and backward on the device -> the bits of y, hn, dgi, dh0."""
    gi, h0 = gi.clone().requires_grad_(), h0.clone().requires_grad_()
    y, hn = dg.gru_scan(gi, w, b, h0)
    ((y * gy).sum() + (hn * ghn).sum()).backward()
    return [t.detach().cpu().numpy().view(np.int32) for t in (y, hn, gi.grad, h0.grad)]


def _scan_inputs(B=33, T=7, H=48, seed=5):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).cuda()  # noqa: E731
    k = H ** -0.5
    return dict(gi=r(B, T, 3 * H), w=r(3 * H, H) * k, b=r(3 * H) * k, h0=r(B, H), gy=r(B, T, H), ghn=r(B, H))


def test_rows_are_independent_and_runs_reproducible():
    a = _scan_inputs()
    full = _scan(a["gi"], a["w"], a["b"], a["h0"], a["gy"], a["ghn"])
    again = _scan(a["gi"], a["w"], a["b"], a["h0"], a["gy"], a["ghn"])
    assert all(np.array_equal(p, q) for p, q in zip(full, again))                       # two runs: the same bits
    row = 20                                                                            # in the second tile
    alone = _scan(a["gi"][row:row + 1].contiguous(), a["w"], a["b"], a["h0"][row:row + 1].contiguous(),
                  a["gy"][row:row + 1].contiguous(), a["ghn"][row:row + 1].contiguous())
    assert all(np.array_equal(p[row:row + 1], q) for p, q in zip(full, alone))          # the row alone
    perm = torch.arange(33)
    perm[3], perm[row] = row, 3                                                         # the row in the first tile, lane 3
    moved = _scan(a["gi"][perm].contiguous(), a["w"], a["b"], a["h0"][perm].contiguous(), a["gy"][perm].contiguous(),
                  a["ghn"][perm].contiguous())
    assert all(np.array_equal(p[row], q[3]) and np.array_equal(p[3], q[row]) for p, q in zip(full, moved))


def test_a_nan_row_stays_in_its_row():
    a = _scan_inputs(B=18, T=6, H=16, seed=6)
    clean = _scan(a["gi"], a["w"], a["b"], a["h0"], a["gy"], a["ghn"])
    gi = a["gi"].clone()
    gi[2, 3, 5] = float("nan")
    dirty = _scan(gi, a["w"], a["b"], a["h0"], a["gy"], a["ghn"])
    rows = [b for b in range(18) if b != 2]
    assert all(np.array_equal(p[rows], q[rows]) for p, q in zip(clean, dirty))          # the other rows: bit-identical
    y = dirty[0].view(np.float32)
    assert np.isnan(y[2, 3:, 5]).all() and np.isnan(y[2, 4:]).all()                     # NaN from its frame on: the unit, then all
    assert np.array_equal(dirty[0][2, :3], clean[0][2, :3])                             # and the frames before it untouched
    assert np.isnan(dirty[1].view(np.float32)[2]).all() and np.isnan(dirty[3].view(np.float32)[2]).all()


def test_saturated_gates_give_no_nan():
    a = _scan_inputs(B=4, T=3, H=16, seed=7)
    gi = a["gi"].clone()
    gi[:, :, 0::2] = 100.0
    gi[:, :, 1::2] = -100.0
    out = _scan(gi, a["w"], a["b"], a["h0"], a["gy"], a["ghn"])
    assert all(np.isfinite(o.view(np.float32)).all() for o in out)


def test_refusals_launch_nothing():
    lib = _capi.load()
    B, T, H = 3, 2, 16
    S = 7.25
    full = lambda *s: torch.full(s, S, device="cuda")  # noqa: E731
    gi, w, b, h0 = torch.randn(B, T, 3 * H, device="cuda"), torch.randn(3 * H, H, device="cuda"), torch.randn(3 * H, device="cuda"), None
    y, hn, res = full(B, T, 144), full(B, 144), full(B, T, 4 * 144)
    dgi, dgh, dh0 = full(B, T, 3 * 144), full(B, T, 3 * 144), full(B, 144)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(B_=B, T_=T, H_=H, gi_=gi, w_=w, y_=y, hn_=hn):
        return lib.wekws_hip_gru_scan_forward(p(gi_), p(w_), p(b), p(h0), B_, T_, H_, p(y_), p(hn_), p(res), s)

    def bwd(B_=B, T_=T, H_=H, y_=y, res_=res, w_=w, dgi_=dgi, dgh_=dgh):
        return lib.wekws_hip_gru_scan_backward(p(gi), None, p(y_), None, p(res_), p(w_), B_, T_, H_, p(dgi_), p(dgh_), p(dh0), s)

    for call in (fwd, bwd):
        for kw in (dict(H_=24), dict(H_=144), dict(H_=8), dict(T_=0), dict(B_=0), dict(w_=None), dict(y_=None)):
            assert call(**kw) == EINVAL, (call.__name__, kw)
            assert "gru_scan" in _capi.last_error()
    assert fwd(gi_=None) == EINVAL and fwd(hn_=None) == EINVAL
    assert bwd(res_=None) == EINVAL and bwd(dgi_=None) == EINVAL and bwd(dgh_=None) == EINVAL
    torch.cuda.synchronize()
    for t in (y, hn, res, dgi, dgh, dh0):
        assert bool((t == S).all())                                                     # the sentinel is untouched
    with pytest.raises(ValueError):
        dg.gru_scan(torch.zeros(1, 1, 72, device="cuda"), torch.zeros(72, 24, device="cuda"), None)   # H = 24: no launch, no fallback


@pytest.mark.parametrize("kw", [dict(bidirectional=True), dict(dropout=0.25, num_layers=2), dict(hidden_size=24)])
def test_unsupported_modules_take_torchs_path(kw, monkeypatch):
    torch.manual_seed(9)
    args = dict(input_size=20, hidden_size=16, num_layers=1, batch_first=True)
    args.update(kw)
    ref = nn.GRU(**args).cuda().eval()
    dev = dg.DeviceGRU(**args).cuda().eval()
    dev.load_state_dict(ref.state_dict())
    monkeypatch.setattr(dg, "gru_scan", lambda *a, **k: pytest.fail("the device path ran"))
    x = torch.randn(3, 5, 20, device="cuda")
    with torch.no_grad():
        (ya, ha), (yb, hb) = ref(x), dev(x)
    assert torch.equal(ya, yb) and torch.equal(ha, hb)


def test_only_what_is_asked_for():
    a = _scan_inputs(B=5, T=4, H=32, seed=8)
    with torch.no_grad():
        y, hn = dg.gru_scan(a["gi"], a["w"], a["b"], a["h0"])
    assert not y.requires_grad and torch.equal(y[:, -1], hn)
    w = a["w"].clone().requires_grad_()
    y2, _ = dg.gru_scan(a["gi"], w, None, None)                                          # no bias, no h0, W_hh's gradient alone
    y2.sum().backward()
    assert w.grad is not None and w.grad.shape == w.shape and bool(torch.isfinite(w.grad).all())
    gi = a["gi"].clone().requires_grad_()
    _, hn3 = dg.gru_scan(gi, a["w"], a["b"], a["h0"])
    hn3.sum().backward()                                                                 # grad_y is NULL
    assert gi.grad is not None and bool(gi.grad.abs().sum() > 0)
