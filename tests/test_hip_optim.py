"""GPU: the optimiser step (wekws_hip_clip_adam_step / wekws_hip_grad_norm, wekws_amd.optim.ClipAdam) on the case matrix of
tests/optim_matrix.py: norm, moments and parameters within the derived bars of the float64 oracle, the state block, the same
bits on every run and beside an MFMA tenant, non-finite gradients, refusals that launch nothing, ClipAdam against torch's
three statements, TrainExecutor without a host read, the state dict both ways with torch.optim.Adam, broken views."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import optim_matrix as om
from tests import optim_ref
from tests.test_hip_tenants import tenant  # noqa: F401  (the MFMA tenants of the second stream)
from tests.train_step import HYPER, _Counter

pytestmark = pytest.mark.gpu

U = om.U
# What the device's own arithmetic allows, in the units of the bars, whatever the reference's error.  First-order rounding
# analysis: a float32 rounding -- of an operation's result or of a hyper-parameter -- is at most half an ulp, which is at most
# one unit (2^-24) of the rounded term:
#   norm  every square exact and every add in double (n 2^-53 relative at worst), one rounding to float32: 1
#   g~    = coef g + wd p: per term its factor (1), its product (1) and the add (1): at most 3 units of ga
#   m'    on beta1 |m|: beta1 (1), the product (1), the add (1) = 3;  on (1 - beta1) ga: 1 - beta1 (1), g~ (3), the product (1), the add (1) = 6
#   v'    on (1 - beta2) ga^2: g~^2 (2 x 3 + 1), 1 - beta2 (1), the product (1), the add (1) = 10;  on beta2 v: 3
# (a fused multiply-add only removes roundings.  p' has no such bound in its units: m' / denom inherits the cancellation of m'.)
DEVICE_BOUND = {"norm": 1.0, "m": 6.0, "v": 10.0}


class _Buffers:
    def __init__(self, case, step0=None):
        from wekws_amd import _capi
        self.lib = _capi.load()
        self.n = int(case["p"].shape[0])
        self.p, self.g, self.m, self.v = (torch.from_numpy(np.array(case[k])).cuda() for k in ("p", "g", "m", "v"))
        self.state = torch.zeros(optim_ref.STATE_BYTES, dtype=torch.uint8, device="cuda")
        self.state.view(torch.int64)[0] = case["step"] if step0 is None else step0
        self.ws = torch.full((optim_ref.plan(self.n)[2],), 0xA5, dtype=torch.uint8, device="cuda")
        self.norm = torch.full((), -1.0, device="cuda")

    def step(self, hyper, skip=1, stream=None, **over):
        k = dict(p=self.p.data_ptr(), g=self.g.data_ptr(), m=self.m.data_ptr(), v=self.v.data_ptr(), n=self.n, state=self.state.data_ptr(),
                 lr=hyper["lr"], b1=hyper["betas"][0], b2=hyper["betas"][1], eps=hyper["eps"], wd=hyper["weight_decay"],
                 clip=hyper["max_norm"], ws=self.ws.data_ptr(), ws_bytes=self.ws.numel())
        k.update(over)
        return self.lib.wekws_hip_clip_adam_step(k["p"], k["g"], k["m"], k["v"], k["n"], k["state"], k["lr"], k["b1"], k["b2"], k["eps"],
                                                 k["wd"], k["clip"], skip, k["ws"], k["ws_bytes"], stream)

    def grad_norm(self, stream=None):
        return self.lib.wekws_hip_grad_norm(self.g.data_ptr(), self.n, self.norm.data_ptr(), self.ws.data_ptr(), self.ws.numel(), stream)

    def read(self):
        st = np.frombuffer(self.state.cpu().numpy().tobytes(), dtype=optim_ref.STATE_DTYPE)[0]
        return dict(p=self.p.cpu().numpy(), g=self.g.cpu().numpy(), m=self.m.cpu().numpy(), v=self.v.cpu().numpy(), state=st)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("p", "g", "m", "v")) and a["state"].tobytes() == b["state"].tobytes()


def _record(error_report, u):
    for k, x in u.items():
        key = f"optim/{k}_units"
        error_report[key] = max(x, error_report.get(key, 0.0))


@pytest.mark.parametrize("name", om.case_names())
def test_step_within_the_bars(error_report, name):
    from wekws_amd import _capi
    c, o = om.load_case(name), om.oracle(name)
    b = _Buffers(c)
    assert b.step(c["hyper"]) == 0, _capi.last_error()
    r = b.read()
    st = r["state"]
    u = om.units(c, o, dict(norm=st["norm_f32"], p=r["p"], m=r["m"], v=r["v"]))
    print(f"{name}: norm {u['norm']:.2f} m {u['m']:.2f} v {u['v']:.2f} p {u['p']:.2f} units (bars {om.BARS})")
    _record(error_report, u)
    assert all(u[k] <= om.BARS[k] for k in u), u
    assert all(u[k] <= DEVICE_BOUND[k] for k in DEVICE_BOUND), u
    assert np.array_equal(_bits(r["g"]), _bits(c["g"]))                                # the gradient is left unscaled
    # the state block
    assert st["step"] == c["step"] + 1 and st["skipped"] == 0 and st["apply"] == 1 and st["finite"] == 1
    assert abs(st["norm"] - o["norm"]) <= (b.n * 2.0 ** -53 + 2.0 ** -52) * o["norm"]  # double adds, one sqrt
    assert st["norm_f32"] == np.float32(st["norm"])
    if o["coef"] == 1.0:
        assert st["coef"] == 1.0
    else:
        assert abs(float(st["coef"]) - o["coef"]) <= U * o["coef"]                     # one rounding to float32
    # pow in double within 4 ulp of a value below 1 (2^-53 each); sqrt(x) moves by dx / (2 sqrt x)
    assert abs(st["bc1"] - o["bc1"]) <= 4 * 2.0 ** -53
    assert abs(st["bc2sqrt"] - o["bc2sqrt"]) <= 4 * 2.0 ** -53 / (2 * o["bc2sqrt"]) + 2.0 ** -53
    assert st["step_size"] == np.float32(c["hyper"]["lr"] / st["bc1"]) and st["bc2sqrt_f32"] == np.float32(st["bc2sqrt"])
    # the norm on its own: the same bits
    assert b.grad_norm() == 0, _capi.last_error()
    assert np.array_equal(_bits(b.norm), _bits(st["norm_f32"]))


@pytest.mark.parametrize("name", ["first_clip_n5", f"s12345_clip_n{2 * om.TILE + 3}", "cancel_n300000",
                                  f"first_clip_n{optim_ref.FOLD_SEG * om.TILE + 5}"])
def test_same_inputs_same_bits(name):
    c = om.load_case(name)
    runs = []
    for _ in range(2):
        b = _Buffers(c)
        assert b.step(c["hyper"]) == 0
        runs.append(b.read())
    assert _same(runs[0], runs[1])
    assert not np.array_equal(runs[0]["p"], c["p"])


def _nonfinite_case(where, value):
    n = om.TILE + 3                                                   # a second tile of three scalars
    rng = np.random.default_rng(5)
    g = (rng.standard_normal(n) / math.sqrt(n)).astype(np.float32)
    g[where] = value
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    m = (0.01 * rng.standard_normal(n)).astype(np.float32)
    v = (1e-4 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    return dict(p=p, g=g, m=m, v=v, step=7, hyper=dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, max_norm=5.0))


@pytest.mark.parametrize("where,value", [(0, float("nan")), (om.TILE + 2, float("nan")), (1234, float("inf"))])
def test_nonfinite_gradient_skips_or_steps(where, value):
    c = _nonfinite_case(where, value)
    b = _Buffers(c)
    before = b.read()
    assert b.step(c["hyper"], skip=1) == 0
    r = b.read()
    assert all(np.array_equal(_bits(r[k]), _bits(before[k])) for k in ("p", "g", "m", "v"))       # nothing written
    st = r["state"]
    assert st["step"] == 7 and st["skipped"] == 1 and st["apply"] == 0 and st["finite"] == 0 and not np.isfinite(st["norm_f32"])
    assert b.step(c["hyper"], skip=1) == 0 and b.read()["state"]["skipped"] == 2
    assert b.step(c["hyper"], skip=0) == 0                            # plain Adam: the step is applied
    r = b.read()
    st = r["state"]
    assert st["step"] == 8 and st["skipped"] == 2 and st["apply"] == 1 and st["finite"] == 0
    assert np.isnan(r["p"][where]) and np.isnan(r["m"][where]) and not np.array_equal(_bits(r["p"]), _bits(before["p"]))
    assert b.grad_norm() == 0 and not np.isfinite(b.norm.item())


def test_a_norm_float32_squares_overflow_is_clipped_and_stepped():
    """Deviation 3, on purpose: g = 1e20 on 1,000 elements has a float32 sum of squares of +Inf and a norm of 3.16e21."""
    rng = np.random.default_rng(6)
    n = 1000
    c = dict(p=(0.1 * rng.standard_normal(n)).astype(np.float32), g=np.full(n, 1e20, np.float32), m=np.zeros(n, np.float32),
             v=np.zeros(n, np.float32), step=0, hyper=dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, max_norm=5.0))
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.sum(c["g"] * c["g"], dtype=np.float32))
    o = optim_ref.oracle_step(c["p"], c["g"], c["m"], c["v"], 0, **c["hyper"])
    b = _Buffers(c)
    assert b.step(c["hyper"], skip=1) == 0
    r = b.read()
    st = r["state"]
    assert st["apply"] == 1 and st["finite"] == 1 and st["step"] == 1 and st["skipped"] == 0 and np.isfinite(st["norm_f32"])
    u = om.units(c, o, dict(norm=st["norm_f32"], p=r["p"], m=r["m"], v=r["v"]))
    print(u)
    assert all(u[k] <= om.BARS[k] for k in u) and all(u[k] <= DEVICE_BOUND[k] for k in DEVICE_BOUND), u


def test_argument_errors_launch_nothing():
    from wekws_amd import _capi
    c = om.load_case("s12345_clip_n8195")
    b = _Buffers(c)
    before = b.read()
    ws_before = b.ws.clone()
    h = c["hyper"]
    nan = float("nan")
    bad = [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(state=None), dict(ws=None), dict(n=0), dict(n=-3),
           dict(n=optim_ref.MAX_ELEMS + 1), dict(p=b.p.data_ptr() + 4), dict(g=b.g.data_ptr() + 8), dict(m=b.m.data_ptr() + 4),
           dict(v=b.v.data_ptr() + 12), dict(state=b.state.data_ptr() + 8), dict(ws=b.ws.data_ptr() + 8), dict(m=b.p.data_ptr() + 16, n=64),
           dict(lr=-1e-3), dict(lr=nan), dict(b1=1.0), dict(b1=-0.5), dict(b2=1.0), dict(b2=nan), dict(eps=-1e-8), dict(wd=-1e-4),
           dict(clip=0.0), dict(clip=-1.0), dict(clip=nan), dict(ws_bytes=b.ws.numel() - 1), dict(ws_bytes=0)]
    for over in bad:
        assert b.step(h, **over) == -1 and _capi.last_error() != "", over
    assert b.lib.wekws_hip_grad_norm(b.g.data_ptr(), 0, b.norm.data_ptr(), b.ws.data_ptr(), b.ws.numel(), None) == -1
    assert b.lib.wekws_hip_grad_norm(b.g.data_ptr(), b.n, b.norm.data_ptr(), b.ws.data_ptr(), 8, None) == -1
    assert b.lib.wekws_hip_grad_norm(b.g.data_ptr() + 4, b.n, b.norm.data_ptr(), b.ws.data_ptr(), b.ws.numel(), None) == -1
    torch.cuda.synchronize()
    assert _same(b.read(), before) and torch.equal(b.ws, ws_before) and float(b.norm) == -1.0


def test_three_kernels_beside_an_mfma_tenant(tenant):  # noqa: F811
    """The step on one stream, an MFMA-heavy forward on another: bit-identical to the solo run."""
    names = ["first_clip_n65", "s12345_clip_n300000", "cancel_n300000", f"first_clip_n{optim_ref.FOLD_SEG * om.TILE + 5}"]
    cases = [om.load_case(n) for n in names]

    def work(stream=None):
        out = []
        for c in cases:
            b = _Buffers(c)
            assert b.step(c["hyper"], stream=stream) == 0 and b.grad_norm(stream) == 0
            out.append(b)
        return out

    solo = [(b.read(), b.norm.clone()) for b in work()]
    tm, tx = tenant
    torch.cuda.synchronize()
    s_a, s_b = torch.cuda.Stream(), torch.cuda.Stream()
    for rnd in range(4):
        with torch.cuda.stream(s_b):
            for _ in range(8):
                tm(tx)
        with torch.cuda.stream(s_a):
            got = work(C.c_void_p(s_a.cuda_stream))
        torch.cuda.synchronize()
        assert all(_same(b.read(), s[0]) and np.array_equal(_bits(b.norm), _bits(s[1])) for b, s in zip(got, solo)), rnd


# ------------------------------------------------------------------------------------------------ ClipAdam
class _CtcHead(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(40, 16)

    def forward(self, x):
        return self.lin(x), None


def _loader(sizes, T, seed, infeasible=()):
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(sizes):
        feats = rng.standard_normal((n, T, 40)).astype(np.float32)
        lengths = rng.integers(T // 2, T + 1, n).astype(np.int32)
        lengths[0] = T
        target = rng.integers(1, 16, (n, 3)).astype(np.int64)
        tl = rng.integers(0, 4, n).astype(np.int32)
        if i in infeasible:
            lengths[1], tl[1] = 2, 3                                     # three labels in two frames
        out.append(dict(keys=[f"utt{i}_{j}" for j in range(n)], feats=torch.from_numpy(feats), target=torch.from_numpy(target),
                        feats_lengths=torch.from_numpy(lengths), target_lengths=torch.from_numpy(tl)))
    return out


def _loss(model, b):
    from wekws_amd.criterion import criterion_device
    logits, _ = model(b["feats"].cuda())
    return criterion_device("ctc", logits, b["target"].cuda(), b["feats_lengths"].cuda(), target_lengths=b["target_lengths"].cuda(),
                            min_duration=0, validation=False).loss


def _p_units(got, want, before):
    """Units of the p' bar between two float32 steps from the same start: the scale is |p| + |the step|."""
    worst = 0.0
    for a, w, b in zip(got, want, before):
        a, w, b = (x.detach().cpu().numpy().astype(np.float64) for x in (a, w, b))
        den = U * (np.abs(b) + np.abs(w - b))
        err = np.abs(a - w)
        assert not np.any(err[den == 0]) and np.isfinite(err).all()
        worst = max(worst, float((err[den > 0] / den[den > 0]).max()) if (den > 0).any() else 0.0)
    return worst


def test_clip_adam_against_torchs_three_statements():
    from wekws_amd.optim import ClipAdam
    torch.manual_seed(3)
    model = _CtcHead().cuda()
    twin = copy.deepcopy(model)
    opt = ClipAdam(model.parameters(), **HYPER)
    ref = torch.optim.Adam(twin.parameters(), **HYPER)
    loader = _loader((7, 9, 5, 6), 12, 17, infeasible=(1,))
    clip = 0.05
    for i, batch in enumerate(loader):
        with torch.no_grad():                                         # the twin starts every batch from the device's state
            for q, p in zip(twin.parameters(), model.parameters()):
                q.copy_(p)
        ref.load_state_dict(opt.state_dict())
        before = [p.detach().clone() for p in model.parameters()]
        opt.zero_grad()
        _loss(model, batch).backward()
        norm = opt.clip_and_step(clip)
        assert norm.shape == () and norm.dtype == torch.float32 and norm.is_cuda
        ref.zero_grad()
        _loss(twin, batch).backward()
        want_norm = torch.nn.utils.clip_grad_norm_(twin.parameters(), clip)
        if torch.isfinite(want_norm):
            ref.step()
            assert abs(float(norm) - float(want_norm)) <= 2 * om.BARS["norm"] * U * float(want_norm)
            assert float(opt.last_clip_coef) < 1.0                    # clipping was active
        else:
            assert i == 1 and not math.isfinite(float(norm))
        u = _p_units(list(model.parameters()), list(twin.parameters()), before)
        print(f"batch {i}: {u:.2f} units between ClipAdam and torch's three statements (bar 2 x {om.BARS['p']})")
        assert u <= 2 * om.BARS["p"]
        assert (i == 1) == all(torch.equal(p, b) for p, b in zip(model.parameters(), before))   # only the skipped batch leaves p alone
    assert int(opt.skipped_steps) == 1 and int(opt.steps) == len(loader) - 1


def test_train_executor_reads_nothing_on_the_host(monkeypatch):
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(4)
    model = _CtcHead().cuda()
    twin = copy.deepcopy(model)
    start = [p.detach().clone() for p in model.parameters()]
    loader = _loader((7, 9, 5), 12, 17, infeasible=(1,))
    args = {"criterion": "ctc", "grad_clip": 5.0, "log_interval": 100}
    opt = ClipAdam(model.parameters(), **HYPER)
    ref = torch.optim.Adam(twin.parameters(), **HYPER)
    TrainExecutor().train(model, opt, loader[:1], "cuda", None, args)           # (the first call of a kernel loads its code object)
    TrainExecutor().train(twin, ref, loader[:1], "cuda", None, args)
    torch.cuda.synchronize()
    with monkeypatch.context() as mp:
        counter = _Counter(mp)
        TrainExecutor().train(model, opt, loader, "cuda", None, args)
        reads = list(counter.calls)
        TrainExecutor().train(twin, ref, loader, "cuda", None, args)
        reads_torch = counter.calls[len(reads):]
    assert reads == [], reads                                                     # no host read in the whole epoch
    assert reads_torch.count("__bool__") >= len(loader)                           # the counter sees the reference's `if`
    assert int(opt.steps) == 1 + len(loader) - 1 and int(opt.skipped_steps) == 1
    assert any(not torch.equal(p, s) for p, s in zip(model.parameters(), start))


def _some_steps(model, opt, loader, clip=None):
    for b in loader:
        opt.zero_grad()
        _loss(model, b).backward()
        if clip is None:
            opt.step()
        else:
            opt.clip_and_step(clip)


def test_state_dict_round_trips_with_torch_adam():
    from wekws_amd.optim import ClipAdam
    loader = _loader((6, 8, 5), 10, 23)
    for first in ("device", "torch"):
        torch.manual_seed(5)
        model = _CtcHead().cuda()
        twin = copy.deepcopy(model)
        mk = {"device": lambda ps: ClipAdam(ps, **HYPER), "torch": lambda ps: torch.optim.Adam(ps, **HYPER)}
        a = mk[first](model.parameters())
        assert a.state_dict()["state"] == {} or first == "torch"
        _some_steps(model, a, loader[:2])                                         # plain step(): a drop-in Adam
        sd = a.state_dict()
        assert sorted(sd["state"]) == [0, 1] and all(float(s["step"]) == 2.0 for s in sd["state"].values())
        assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and sd["state"][0]["exp_avg"].shape == (16, 40)
        with torch.no_grad():
            for q, p in zip(twin.parameters(), model.parameters()):
                q.copy_(p)
        b = mk["torch" if first == "device" else "device"](twin.parameters())
        b.load_state_dict(copy.deepcopy(sd))
        before = [p.detach().clone() for p in model.parameters()]
        _some_steps(model, a, loader[2:])
        _some_steps(twin, b, loader[2:])
        u = _p_units(list(model.parameters()), list(twin.parameters()), before)
        print(f"{first} first: {u:.2f} units after one step from the loaded state")
        assert u <= 2 * om.BARS["p"] and any(not torch.equal(p, s) for p, s in zip(model.parameters(), before))
        sb = b.state_dict()
        assert all(float(s["step"]) == 3.0 for s in sb["state"].values())
        if first == "torch":
            assert int(b.steps) == 3 and int(b.skipped_steps) == 0
            sd["state"][1]["step"] = torch.tensor(5.0)
            with pytest.raises(ValueError, match="steps differ"):
                b.load_state_dict(sd)
            del sd["state"][1]
            with pytest.raises(ValueError, match="no state for parameter 1"):
                b.load_state_dict(sd)


def test_lr_is_read_at_every_step():
    from wekws_amd.optim import ClipAdam
    torch.manual_seed(6)
    model = _CtcHead().cuda()
    opt = ClipAdam(model.parameters(), **HYPER)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.5, patience=0)
    loader = _loader((6, 8), 10, 29)
    _some_steps(model, opt, loader[:1], clip=5.0)
    st = np.frombuffer(opt._state.cpu().numpy().tobytes(), dtype=optim_ref.STATE_DTYPE)[0]
    assert st["step_size"] == np.float32(1e-3 / st["bc1"])
    sched.step(1.0)
    sched.step(2.0)                                                                # worse: the rate halves
    assert opt.param_groups[0]["lr"] == 5e-4
    _some_steps(model, opt, loader[1:], clip=5.0)
    st = np.frombuffer(opt._state.cpu().numpy().tobytes(), dtype=optim_ref.STATE_DTYPE)[0]
    assert st["step"] == 2 and st["step_size"] == np.float32(5e-4 / st["bc1"])


def test_broken_views_raise_and_zero_grad_keeps_them():
    from wekws_amd.optim import ClipAdam
    loader = _loader((6,), 10, 31)

    def fresh():
        torch.manual_seed(7)
        model = _CtcHead().cuda()
        return model, ClipAdam(model.parameters(), **HYPER)

    model, opt = fresh()
    _some_steps(model, opt, loader, clip=5.0)
    opt.zero_grad(set_to_none=True)                                               # the optimiser's own: one zero_() of the flat gradient
    assert all(p.grad is not None and not p.grad.any() for p in model.parameters()) and not opt.flat_grads.any()
    _some_steps(model, opt, loader, clip=5.0)
    model.float().to("cuda")                                                      # already float32 on the device: nothing moves
    _some_steps(model, opt, loader, clip=5.0)
    assert int(opt.steps) == 3
    model.lin.weight.grad = None
    with pytest.raises(RuntimeError, match="flat buffers"):
        opt.clip_and_step(5.0)
    with pytest.raises(RuntimeError, match="flat buffers"):
        opt.step()
    assert int(opt.steps) == 3
    for move in (lambda m: m.cpu().to("cuda"), lambda m: m.double().float(), lambda m: m.zero_grad(set_to_none=True)):
        model, opt = fresh()
        _some_steps(model, opt, loader, clip=5.0)
        flat = opt.flat_params.clone()
        move(model)                                                               # new storage for the data or no gradient at all
        with pytest.raises(RuntimeError, match="flat buffers"):
            opt.clip_and_step(5.0)
        assert torch.equal(opt.flat_params, flat) and int(opt.steps) == 1         # never steps buffers the model no longer uses
