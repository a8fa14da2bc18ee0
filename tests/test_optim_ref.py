"""CPU: the float64 oracle of the optimiser step (tests/optim_ref.py) against torch's own float32 step and the derivation of
the bars (tests/optim_matrix.py); wekws_hip_optim_plan and the refusals of the step calls that need no device, against a
Python restatement of csrc/optim_plan.h; the flattening helper of wekws_amd.optim on CPU tensors."""
import copy
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import optim_matrix as om
from tests import optim_ref
from tests.helpers import pow2_at_or_above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def reference_units(name):
    """Units of torch's float32 CPU step against the oracle, computed once a case."""
    c = om.load_case(name)
    got = optim_ref.torch_step(c["p"], c["g"], c["m"], c["v"], c["step"], **c["hyper"])
    return om.units(c, om.oracle(name), got)


def test_matrix_holds_the_cases_it_names():
    names = om.case_names()
    assert len(names) == len(set(names))
    for n in om.LENGTHS:
        assert f"first_clip_n{n}" in names and f"s12345_clip_n{n}" in names
    for s in om.SCENARIOS:
        assert f"{s}_n300000" in names and f"{s}_n65" in names
    t = optim_ref.plan(om.LENGTHS[-2])[1]
    assert t == optim_ref.FOLD_SEG + 1 and optim_ref.plan(2 * om.TILE + 3)[1] == 3          # the second stage; a third tile of 3 floats
    for name in names:
        c, o = om.load_case(name), om.oracle(name)
        clip = name.startswith(("first_clip", "s12345_clip"))
        assert (o["coef"] < 0.5) if clip else (o["coef"] == 1.0), (name, o["coef"])
        assert (c["step"] == 0) == (not c["m"].any() and not c["v"].any())
    c = om.load_case("zero7_n65")
    assert not c["g"][::7].any() and c["g"][1::7].all()
    c, o = om.load_case("cancel_n300000"), om.oracle("cancel_n300000")
    assert np.abs(o["m"]).max() < 1e-2 * np.abs(c["m"]).max()                               # m' cancels
    c, o = om.load_case("s12345_clip_n300000"), om.oracle("s12345_clip_n300000")
    assert np.median(np.abs(o["p"] - c["p"])[::97]) > 50 * c["hyper"]["lr"]                       # updates far larger than lr
    c, o = om.load_case("tiny_grad_n65"), om.oracle("tiny_grad_n65")
    assert np.sqrt(o["v"]).max() < c["hyper"]["eps"]                                        # eps dominates


def test_oracle_against_a_hand_step():
    o = optim_ref.oracle_step([1.0, -2.0], [3.0, 4.0], [0.0, 0.0], [0.0, 0.0], 0, 0.5, (0.5, 0.75), 0.0, 0.0, 2.5)
    assert o["norm"] == 5.0 and abs(o["coef"] - 2.5 / (5 + 1e-6)) < 1e-15
    # the first step of Adam without eps moves every element by lr against its gradient's sign
    assert np.allclose(o["p"], [0.5, -2.5], rtol=0, atol=1e-15) and o["bc1"] == 0.5 and o["bc2sqrt"] == 0.5
    o = optim_ref.oracle_step([1.0], [3.0], [0.0], [0.0], 0, 0.5, (0.5, 0.75), 0.0, 0.0, math.inf)
    assert o["coef"] == 1.0 and o["m"][0] == 1.5 and o["v"][0] == 2.25


@pytest.mark.parametrize("name", om.case_names())
def test_torch_float32_step_is_near_the_oracle(name):
    u = reference_units(name)
    print(f"{name}: reference units norm {u['norm']:.2f} m {u['m']:.2f} v {u['v']:.2f} p {u['p']:.2f}")
    assert all(u[k] <= om.BARS[k] / 4 for k in u), u


def test_bars_follow_from_the_reference_error():
    worst = {k: max((reference_units(n)[k], n) for n in om.case_names()) for k in om.BARS}
    print({k: (round(v[0], 2), v[1]) for k, v in worst.items()})
    for k, bar in om.BARS.items():
        ref = worst[k][0]
        assert abs(ref - om.REF_UNITS[k]) < 0.01, (k, worst[k])
        assert bar == pow2_at_or_above(4 * ref), (k, ref, bar)


def test_units_see_an_error_and_a_nonzero_where_zero_is_due():
    name = "zero7_n65"
    c, o = om.load_case(name), om.oracle(name)
    got = {k: np.array(o[k]) for k in ("norm", "p", "m", "v")}
    assert om.units(c, o, got) == dict(norm=0.0, m=0.0, v=0.0, p=0.0)
    got["p"][3] += 3 * om.U * (abs(c["p"][3]) + abs(o["p"][3] - c["p"][3]))
    assert abs(om.units(c, o, got)["p"] - 3.0) < 1e-6
    got["v"][5] = np.nan
    assert om.units(c, o, got)["v"] == float("inf")
    z = dict(p=np.zeros(4, np.float32), g=np.zeros(4, np.float32), m=np.zeros(4, np.float32), v=np.zeros(4, np.float32), step=3,
             hyper=c["hyper"])
    oz = optim_ref.oracle_step(z["p"], z["g"], z["m"], z["v"], 3, **z["hyper"])
    assert not oz["p"].any() and om.units(z, oz, dict(norm=0.0, p=oz["p"], m=oz["m"], v=oz["v"]))["m"] == 0.0
    assert om.units(z, oz, dict(norm=0.0, p=oz["p"], m=oz["m"] + 1e-30, v=oz["v"]))["m"] == float("inf")


# ------------------------------------------------------------------------------------------------ the plan and the refusals
def test_plan_matches_the_restatement():
    from wekws_amd import _capi
    lib = _capi.load()
    src = open(os.path.join(ROOT, "wekws_amd", "csrc", "optim_plan.h")).read()
    assert f"kOptimTileFloats = {optim_ref.TILE_FLOATS};" in src and f"kOptimFoldSeg = {optim_ref.FOLD_SEG};" in src
    assert lib.wekws_hip_optim_state_bytes() == optim_ref.STATE_BYTES == optim_ref.STATE_DTYPE.itemsize
    T, S = optim_ref.TILE_FLOATS, optim_ref.FOLD_SEG
    out = (C.c_int64 * 3)()
    for n in (1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 3, S * T, S * T + 1, 300000, 2 * S * T + 1, optim_ref.MAX_ELEMS - 1, optim_ref.MAX_ELEMS):
        assert lib.wekws_hip_optim_plan(n, out) == 0, _capi.last_error()
        assert tuple(out) == optim_ref.plan(n), n
        assert out[2] % 16 == 0 and out[2] >= 8 * out[1]
    assert optim_ref.plan(S * T)[2] == 8 * S and optim_ref.plan(S * T + 1)[2] == (8 * (S + 1 + 2) + 15) // 16 * 16
    assert optim_ref.plan(optim_ref.MAX_ELEMS)[2] == 8 * (S * S + S)
    for n in (0, -1, optim_ref.MAX_ELEMS + 1, 1 << 40):
        assert optim_ref.plan(n) is None
        assert lib.wekws_hip_optim_plan(n, out) == -1 and "n=" in _capi.last_error()
    assert lib.wekws_hip_optim_plan(5, None) == -1 and "NULL" in _capi.last_error()


def test_argument_errors_return_einval_without_a_device():
    from wekws_amd import _capi
    lib = _capi.load()
    step, norm = lib.wekws_hip_clip_adam_step, lib.wekws_hip_grad_norm
    a, b, c, d, st, ws = (4096 * (i + 1) for i in range(6))          # non-NULL, aligned, apart: nothing is dereferenced
    ok = dict(params=a, grads=b, m=c, v=d, n=64, state=st, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-4, clip=5.0, skip=1, ws=ws,
              ws_bytes=16)

    def call(**kw):
        k = dict(ok, **kw)
        return step(k["params"], k["grads"], k["m"], k["v"], k["n"], k["state"], k["lr"], k["b1"], k["b2"], k["eps"], k["wd"], k["clip"],
                    k["skip"], k["ws"], k["ws_bytes"], None)

    for key in ("params", "grads", "m", "v", "state", "ws"):
        assert call(**{key: None}) == -1 and "NULL" in _capi.last_error(), key
        assert call(**{key: ok[key] + 4}) == -1 and "aligned" in _capi.last_error(), key
    for n in (0, -5, optim_ref.MAX_ELEMS + 1):
        assert call(n=n) == -1 and "n=" in _capi.last_error()
    assert call(m=a + 16) == -1 and "overlap" in _capi.last_error()
    assert call(grads=d) == -1 and "overlap" in _capi.last_error()
    nan, inf = float("nan"), float("inf")
    for key, bad, word in (("lr", -1e-3, "lr"), ("lr", nan, "lr"), ("lr", inf, "lr"), ("b1", 1.0, "betas"), ("b1", -0.1, "betas"),
                           ("b2", 1.0, "betas"), ("b2", nan, "betas"), ("eps", -1e-8, "eps"), ("eps", nan, "eps"),
                           ("wd", -1e-4, "weight_decay"), ("wd", nan, "weight_decay"), ("clip", 0.0, "max_norm"),
                           ("clip", -5.0, "max_norm"), ("clip", nan, "max_norm")):
        assert call(**{key: bad}) == -1 and word in _capi.last_error(), (key, bad, _capi.last_error())
    assert call(ws_bytes=15) == -1 and "workspace" in _capi.last_error()
    assert call(n=2 * optim_ref.TILE_FLOATS + 3, ws_bytes=16) == -1 and "workspace" in _capi.last_error()      # three tiles: 32 bytes
    out = 4096 * 9
    assert norm(None, 64, out, ws, 16, None) == -1 and norm(b, 64, None, ws, 16, None) == -1 and norm(b, 64, out, None, 16, None) == -1
    assert norm(b, 0, out, ws, 16, None) == -1 and "n=" in _capi.last_error()
    assert norm(b + 4, 64, out, ws, 16, None) == -1 and "aligned" in _capi.last_error()
    assert norm(b, 64, out, ws, 8, None) == -1 and "workspace" in _capi.last_error()


# ------------------------------------------------------------------------------------------------ the flattening helper
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(5, 7)
        self.b = torch.nn.Linear(7, 3, bias=False)
        self.scale = torch.nn.Parameter(torch.ones(()))

    def forward(self, x):
        return self.b(torch.relu(self.a(x))) * self.scale


def _adopt(net):
    from wekws_amd.optim import FlatViews
    ps = list(net.parameters())
    fv = FlatViews([tuple(p.shape) for p in ps])
    flat = torch.zeros(2, fv.total)
    fv.adopt(ps, flat[0], flat[1])
    return fv, ps, flat


def test_flat_views_offsets_and_views():
    from wekws_amd.optim import ALIGN_ELEMS, FlatViews
    torch.manual_seed(0)
    net = _Net()
    before = [p.detach().clone() for p in net.parameters()]
    fv, ps, flat = _adopt(net)
    assert fv.numels == [1, 35, 7, 21] and fv.offsets == [0, 16, 64, 80] and fv.total == 112   # (scale, a.weight, a.bias, b.weight)
    assert all(o % ALIGN_ELEMS == 0 for o in fv.offsets) and fv.total % ALIGN_ELEMS == 0
    for p, b, o, n in zip(ps, before, fv.offsets, fv.numels):
        assert torch.equal(p.detach(), b) and p.shape == b.shape                   # the values moved with the data
        assert p.data_ptr() == flat[0].data_ptr() + 4 * o and p.grad.data_ptr() == flat[1].data_ptr() + 4 * o
        assert torch.equal(flat[0, o:o + n], b.reshape(-1))
    gaps = torch.ones(fv.total, dtype=torch.bool)
    for o, n in zip(fv.offsets, fv.numels):
        gaps[o:o + n] = False
    assert not flat[:, gaps].any()                                                 # the gaps are zero in both buffers
    assert FlatViews([()]).total == ALIGN_ELEMS and fv.broken(ps, flat[0], flat[1]) == []
    with torch.no_grad():
        flat[0, 64] = 42.0                                                         # the flat buffer IS the parameter
    assert float(net.a.bias[0]) == 42.0


def test_gradients_accumulate_into_the_flat_buffer():
    torch.manual_seed(1)
    net = _Net()
    twin = copy.deepcopy(net)
    fv, ps, flat = _adopt(net)
    x = torch.randn(4, 5)
    for _ in range(2):                                                             # the second backward accumulates
        net(x).square().sum().backward()
        twin(x).square().sum().backward()
    assert fv.broken(ps, flat[0], flat[1]) == []                                   # every p.grad still lies inside the flat buffer
    for p, q, o, n in zip(ps, twin.parameters(), fv.offsets, fv.numels):
        assert torch.equal(p.grad, q.grad) and torch.equal(flat[1, o:o + n], q.grad.reshape(-1))
    flat[1].zero_()
    assert all(not p.grad.any() for p in ps) and fv.broken(ps, flat[0], flat[1]) == []


def test_broken_views_are_detected():
    torch.manual_seed(2)
    net = _Net()
    fv, ps, flat = _adopt(net)
    net.a.weight.grad = None
    bad = fv.broken(ps, flat[0], flat[1])
    assert len(bad) == 1 and "parameter 1" in bad[0] and "None" in bad[0]
    net.a.weight.grad = torch.zeros_like(net.a.weight)
    assert "no longer a view of the flat gradient" in fv.broken(ps, flat[0], flat[1])[0]
    fv, ps, flat = _adopt(net)
    assert fv.broken(ps, flat[0], flat[1]) == []
    net.zero_grad(set_to_none=True)                                                # the module's own zero_grad drops the views
    assert len(fv.broken(ps, flat[0], flat[1])) == 4
    fv, ps, flat = _adopt(net)
    net.double().float()                                                           # what model.to(...) does: new storage for the data
    bad = fv.broken(ps, flat[0], flat[1])
    assert bad and all("data is no longer a view" in b or ".grad" in b for b in bad) and any("data" in b for b in bad)


def test_clip_adam_refuses_what_it_does_not_support():
    from wekws_amd.optim import ClipAdam
    net = _Net()
    with pytest.raises(ValueError, match="ROCm device"):
        ClipAdam(net.parameters())
    with pytest.raises(ValueError, match="amsgrad"):
        ClipAdam(net.parameters(), amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad and maximize"):
        ClipAdam(net.parameters(), maximize=True)
    with pytest.raises(ValueError, match="one parameter group"):
        ClipAdam([{"params": net.a.parameters()}, {"params": net.b.parameters()}])
    with pytest.raises(TypeError, match="float32"):
        ClipAdam(_Net().double().parameters())
    with pytest.raises(ValueError, match="beta"):
        ClipAdam(net.parameters(), betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="learning rate"):
        ClipAdam(net.parameters(), lr=-1.0)
    assert issubclass(ClipAdam, torch.optim.Optimizer)
