"""GPU: wekws_amd.model.batchnorm -- ``DeviceBatchNorm1d`` against its torch twin and the float64 oracle, one forward / backward and
three ``TrainExecutor`` steps (max_pooling, ClipAdam) of a tiny DS-TCN and a tiny MDTC with device BatchNorms against torch's
(float32 and float64), no host read in the step, and the trained state dict served by the packed inference model."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import batchnorm_matrix as bm
from tests.helpers import pow2_at_or_above, tol_for
from tests.train_step import (ARGS, BACKBONES, HDIM, HYPER, IDIM, ODIM, SWAPPED, Kws, _bound, _Counter, _distances, _Float64, _grad_errors,
                              _loader)
from wekws_amd.model import batchnorm

pytestmark = pytest.mark.gpu


def _module(c, cls):
    C = c["x"].shape[1]
    bn = cls(C, eps=bm.EPS, momentum=c["momentum"], affine=c["w"] is not None, track_running_stats=c["rm"] is not None).cuda()
    with torch.no_grad():
        if c["w"] is not None:
            bn.weight.copy_(torch.from_numpy(c["w"].copy()))
            bn.bias.copy_(torch.from_numpy(c["b"].copy()))
        if c["rm"] is not None:
            bn.running_mean.copy_(torch.from_numpy(c["rm"].copy()))
            bn.running_var.copy_(torch.from_numpy(c["rv"].copy()))
            bn.num_batches_tracked.fill_(c["tracked"])
    return bn.train(c["training"])


def _module_results(bn, c):
    t = lambda a: torch.from_numpy(a.copy()).cuda()  # noqa: E731
    x = t(c["x"]).requires_grad_()
    res = t(c["res"]).requires_grad_() if c["res"] is not None else None
    if isinstance(bn, batchnorm.DeviceBatchNorm1d):
        y = bn(x, residual=res, relu=c["relu"])
    else:
        y = bn(x)
        y = y + res if res is not None else y
        y = F.relu(y) if c["relu"] else y
    y.backward(t(c["g"]))
    out = dict(y=y.detach(), dx=x.grad)
    if res is not None:
        out["dres"] = res.grad
    if bn.affine:
        out.update(dw=bn.weight.grad, db=bn.bias.grad)
    if c["calls"] == 2:
        with torch.no_grad():
            bn(t(c["x2"]))
        out.update(rm=bn.running_mean, rv=bn.running_var)
    tracked = int(bn.num_batches_tracked) if bn.track_running_stats else None
    return {k: v.cpu().numpy() for k, v in out.items()}, tracked


@pytest.mark.parametrize("name", ["g_ds", "g_dsd", "g_bn2", "g_bn2_eval", "t129", "f11100", "f01001", "f10010", "mom_none", "mom_1", "off4096",
                                  "fold9"])
def test_device_module_and_torch_module_against_the_oracle(name):
    c = bm.load_case(name)
    dev = _module(c, batchnorm.DeviceBatchNorm1d)
    twin = _module(c, nn.BatchNorm1d)
    assert list(dev.state_dict()) == list(twin.state_dict())
    got, tracked = _module_results(dev, c)
    want, tracked_t = _module_results(twin, c)
    ud, bad_d = bm.units(name, got)
    ut, bad_t = bm.units(name, want)
    print(f"{name}: device {ud}  torch on the device {ut}")
    assert not bad_d and not bad_t and tracked == tracked_t == bm.oracle(name)[2]
    assert all(ud[k] <= bm.BARS[k] for k in ud), ud


def test_only_the_gradients_asked_for_and_what_raises():
    c = bm.load_case("g_bn2")
    t = lambda a: torch.from_numpy(a.copy()).cuda()  # noqa: E731
    g = t(c["g"])
    full = None
    for wx, ww, wb, wr in ((1, 1, 1, 1), (0, 1, 1, 0), (1, 0, 0, 0), (0, 0, 1, 0), (0, 1, 0, 1), (0, 0, 0, 1)):
        x, w, b, r = (t(c[k]).requires_grad_(bool(f)) for k, f in (("x", wx), ("w", ww), ("b", wb), ("res", wr)))
        y = batchnorm.batch_norm_act(x, w, b, t(c["rm"]), t(c["rv"]), torch.tensor(3, device="cuda"), True, 0.1, bm.EPS, relu=True, residual=r)
        y.backward(g)
        grads = (x.grad, w.grad, b.grad, r.grad)
        assert [v is not None for v in grads] == [bool(f) for f in (wx, ww, wb, wr)]
        full = full or grads
        assert all(v is None or torch.equal(v, f) for v, f in zip(grads, full))   # a subset has the full call's bits
    x = t(c["x"]).requires_grad_()
    with torch.no_grad():
        assert not batchnorm.batch_norm_act(x, None, None, None, None, None, True, 0.1, bm.EPS).requires_grad
    # differentiable once
    y = batchnorm.batch_norm_act(x, None, None, None, None, None, True, 0.1, bm.EPS, relu=True)
    gx, = torch.autograd.grad(y, x, g, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    # a (B, C) input is T = 1; one value per channel in training is torch's ValueError, here and in the module
    x2 = t(c["x"][:, :, 0])
    y2 = batchnorm.batch_norm_act(x2, None, None, None, None, None, True, 0.1, bm.EPS)
    assert y2.shape == x2.shape and torch.allclose(y2, F.batch_norm(x2, None, None, training=True, eps=bm.EPS), atol=1e-5)
    bn = batchnorm.DeviceBatchNorm1d(6).cuda()
    for bad in (x2[:1], t(c["x"])[:1, :, :1]):
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            bn(bad)
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            nn.BatchNorm1d(6).cuda()(bad)
    for kw in (dict(eps=0.0), dict(momentum=1.5)):
        with pytest.raises(ValueError):
            batchnorm.batch_norm_act(x, None, None, t(c["rm"]), t(c["rv"]), None, True, **{**dict(momentum=0.1, eps=bm.EPS), **kw})
    with pytest.raises(ValueError):
        batchnorm.batch_norm_act(x, None, None, None, None, None, False, 0.1, bm.EPS)          # eval without buffers
    with pytest.raises(ValueError):
        batchnorm.batch_norm_act(x.cpu(), None, None, None, None, None, True, 0.1, bm.EPS)     # no CPU fallback


@pytest.mark.parametrize("kind", sorted(BACKBONES))
def test_one_forward_backward_against_float64(kind, error_report):
    """One forward / backward in train() from one initialisation: with device BatchNorms, with torch's in float32 and with
    torch's in float64.  For every parameter tensor the device path's gradient error against the float64 run is at most
    pow2_at_or_above(4 x the float32 torch path's); the running buffers are held to the same rule."""
    torch.manual_seed(11)
    base = Kws(BACKBONES[kind][0]())
    x = torch.randn(6, 12, IDIM)
    sel = torch.randn(6, 12, ODIM)
    models = {"dev": copy.deepcopy(base).cuda(), "t32": copy.deepcopy(base).cuda(), "t64": copy.deepcopy(base).double().cuda()}
    assert batchnorm.use_device_batchnorms(models["dev"]) == SWAPPED[kind]
    assert sum(isinstance(m, batchnorm.DeviceBatchNorm1d) for m in models["t32"].modules()) == 0
    for tag, m in models.items():
        m.train()
        dt = torch.float64 if tag == "t64" else torch.float32
        y, _ = m(x.to("cuda", dt))
        (y * sel.to("cuda", dt)).sum().backward()
    names = [n for n, _ in base.named_parameters()] + [n for n, b in base.named_buffers() if b.dtype.is_floating_point]
    e_ref = _grad_errors(models["t32"], models["t64"], names)
    e_dev = _grad_errors(models["dev"], models["t64"], names)
    worst = 0.0
    for n in names:
        bound = _bound(e_ref[n])
        print(f"{kind}: {n}: float32 torch path {e_ref[n]:.3g} units from float64 -> bound {bound:.3g}; device BatchNorms {e_dev[n]:.3g}")
        worst = max(worst, e_dev[n] / bound if bound > 0 else float(e_dev[n] > 0))
    error_report[f"batchnorm_train/{kind}/worst_fraction_of_bound"] = worst
    for n in names:
        assert e_dev[n] <= _bound(e_ref[n]), (n, e_dev[n], e_ref[n])
    for m in (models["dev"], models["t32"]):
        assert all(int(b) == 1 for n, b in m.named_buffers() if n.endswith("num_batches_tracked"))


@pytest.mark.parametrize("kind", sorted(BACKBONES))
def test_three_training_steps_with_device_batchnorms_and_with_torch_batchnorms(kind, error_report):
    """Three TrainExecutor steps (max_pooling criterion, ClipAdam, dropout 0) from one initialisation, the rule of
    tests/test_hip_conv_train.py: the distance between the run with device BatchNorms and the float32 run with torch's is at
    most pow2_at_or_above(4 x the float32 torch path's distance from the float64 run), in units of 2^-24 (|p0| + |p64 - p0|)
    per element; the running buffers under the same rule, in units of 2^-24 |b64|."""
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(7)
    base = Kws(BACKBONES[kind][0]())
    loader = _loader((6, 8, 5), 12, 31)
    start = [p.detach().clone() for p in base.parameters()]
    m_dev = copy.deepcopy(base).cuda()
    assert batchnorm.use_device_batchnorms(m_dev) == SWAPPED[kind]
    m_t32 = copy.deepcopy(base).cuda()
    m_t64 = _Float64(copy.deepcopy(base)).cuda()
    TrainExecutor().train(m_dev, ClipAdam(m_dev.parameters(), **HYPER), loader, "cuda", None, ARGS)
    TrainExecutor().train(m_t32, ClipAdam(m_t32.parameters(), **HYPER), loader, "cuda", None, ARGS)
    TrainExecutor().train(m_t64, torch.optim.Adam(m_t64.parameters(), **HYPER), loader, "cuda", None, ARGS)
    p_dev, p_t32, p_t64 = (list(m.parameters()) for m in (m_dev, m_t32, m_t64))
    assert any(not torch.equal(p.cpu(), s) for p, s in zip(p_dev, start))
    d_ref = max(_distances(p_t32, p_t64, start, p_t64))
    d_dev = max(_distances(p_dev, p_t32, start, p_t64))
    bound = pow2_at_or_above(4 * d_ref)
    print(f"{kind}: float32 torch path from float64: {d_ref:.3g} units -> bound {bound:.3g}; device BatchNorms from torch's: {d_dev:.3g} units")
    error_report[f"batchnorm_train/{kind}/torch32_from_float64"] = d_ref
    error_report[f"batchnorm_train/{kind}/device_from_torch32"] = d_dev
    assert d_dev <= bound, (d_dev, d_ref, bound)
    fb = lambda m: [b for _, b in m.named_buffers() if b.dtype.is_floating_point]  # noqa: E731
    zeros = [torch.zeros_like(b) for b in fb(m_t64)]
    b_ref = max(_distances(fb(m_t32), fb(m_t64), zeros, fb(m_t64)))
    b_dev = max(_distances(fb(m_dev), fb(m_t32), zeros, fb(m_t64)))
    print(f"{kind}: running buffers: float32 torch path from float64 {b_ref:.3g} units, device from torch's {b_dev:.3g}")
    assert b_dev <= pow2_at_or_above(4 * b_ref), (b_dev, b_ref)
    assert all(int(b) == 3 for n, b in m_dev.named_buffers() if n.endswith("num_batches_tracked"))


@pytest.mark.parametrize("kind", sorted(BACKBONES))
def test_training_step_reads_nothing_on_the_host(kind, monkeypatch):
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(8)
    model = Kws(BACKBONES[kind][0]()).cuda()
    assert batchnorm.use_device_batchnorms(model) == SWAPPED[kind]
    start = [p.detach().clone() for p in model.parameters()]
    loader = _loader((6, 8, 5), 12, 32)
    opt = ClipAdam(model.parameters(), **HYPER)
    TrainExecutor().train(model, opt, loader[:1], "cuda", None, ARGS)           # (the first call of a kernel loads its code object)
    torch.cuda.synchronize()
    with monkeypatch.context() as mp:
        counter = _Counter(mp)
        TrainExecutor().train(model, opt, loader, "cuda", None, ARGS)
        reads = list(counter.calls)
    assert reads == [], reads
    assert int(opt.steps) == 1 + len(loader) and int(opt.skipped_steps) == 0
    assert any(not torch.equal(p, s) for p, s in zip(model.parameters(), start))
    assert all(int(b) == 1 + len(loader) for n, b in model.named_buffers() if n.endswith("num_batches_tracked"))


@pytest.mark.parametrize("kind", sorted(BACKBONES))
def test_trained_state_dict_is_served_by_the_packed_model(kind):
    """train -> pack -> serve: the state dict of the model trained with device BatchNorms, buffers included, loads into
    init_model's packed KWSModel, whose posteriors agree with the module's in eval() at the bar of tests/test_hip_parity.py."""
    from wekws_amd.model.kws_model import init_model
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(9)
    make, bb_cfg = BACKBONES[kind]
    model = Kws(make()).cuda()
    twin = copy.deepcopy(model)
    assert batchnorm.use_device_batchnorms(model) == SWAPPED[kind] and list(model.state_dict()) == list(twin.state_dict())
    TrainExecutor().train(model, ClipAdam(model.parameters(), **HYPER), _loader((6, 8, 5), 12, 33), "cuda", None, ARGS)
    assert any(not torch.equal(a, b) for (n, a), b in zip(model.named_buffers(), twin.buffers()) if n.endswith("running_mean"))
    cfg = dict(input_dim=IDIM, output_dim=ODIM, hidden_dim=HDIM, preprocessing=dict(type="linear"), backbone=bb_cfg)
    packed = init_model(cfg)
    packed.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    packed = packed.cuda().eval()
    x = torch.randn(4, 30, IDIM, device="cuda")
    model.eval()
    twin.load_state_dict(model.state_dict())
    twin.eval()
    with torch.no_grad():
        want, cache = model(x)                                                   # the fused eval kernels
        want_t, _ = twin(x)                                                      # torch's BatchNorms on the same state
    y, pc = packed(x)
    err, err_t = float((y - want).abs().max()), float((want - want_t).abs().max())
    cerr = float((pc - cache).abs().max())
    print(f"{kind}: packed posteriors vs the trained module: max|err| = {err:.2e} (bar {tol_for(want.cpu().numpy()):.1e}), cache {cerr:.2e}; "
          f"device BatchNorms vs torch's in eval(): {err_t:.2e}")
    assert y.shape == want.shape and err <= tol_for(want.cpu().numpy()) and err_t <= tol_for(want.cpu().numpy())
    assert pc.shape == cache.shape and cerr <= tol_for(cache.cpu().numpy())
