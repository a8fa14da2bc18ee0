"""GPU: a tiny CnnBlock TCN (dropout 0) under a Linear front and classifier with ``use_device_dense_convs`` and
``use_device_batchnorms`` on, under the set-up and the rule of tests/test_hip_pointwise_train_step.py: one forward / backward per
parameter and three ``TrainExecutor`` steps (max_pooling, ClipAdam) against the unswapped float32 torch path and a float64 run, no
host read in the step, and the trained state dict served by the packed inference model (``type: tcn``, ``ds: false``)."""
import copy

import pytest
import torch

from tests.helpers import pow2_at_or_above, tol_for
from tests.train_step import ARGS, HDIM, HYPER, IDIM, ODIM, Kws, _bound, _Counter, _distances, _Float64, _grad_errors, _loader
from wekws_amd.model import batchnorm, dense, depthwise, pointwise, tcn

pytestmark = pytest.mark.gpu

LAYERS, TAPS = 2, 3
BACKBONE_CFG = dict(type="tcn", ds=False, num_layers=LAYERS, kernel_size=TAPS, dropout=0.0)


def _base():
    return Kws(tcn.TCN(LAYERS, HDIM, TAPS, dropout=0.0, block_class=tcn.CnnBlock))


def _device(base):
    """A copy of ``base`` (torch's convolutions and BatchNorms) on the device with every swap that finds something on."""
    m = copy.deepcopy(base).cuda()
    assert dense.use_device_dense_convs(m) == LAYERS
    assert batchnorm.use_device_batchnorms(m) == LAYERS
    assert pointwise.use_device_pointwise_convs(m) == 0 and depthwise.use_device_depthwise_convs(m) == 0
    assert sum(type(c) is dense.DenseConv1d for c in m.modules()) == LAYERS
    return m


def test_one_forward_backward_against_float64(error_report):
    """One forward / backward in train() from one initialisation: with the swaps on, with torch's modules in float32 and with
    torch's in float64.  For every parameter tensor the device path's gradient error against the float64 run is at most
    pow2_at_or_above(4 x the float32 torch path's); the running buffers are held to the same rule.  Measured on MI355X, the
    tensor closest to its bound: preprocessing.out.0.bias 4.47 units (torch path 3.75, bound 16); the convolutions' biases, in front
    of a training-mode BatchNorm, have an exact gradient of zero and hold rounding noise in both paths (3e15 .. 1e16 units)."""
    torch.manual_seed(11)
    base = _base()
    x = torch.randn(6, 12, IDIM)
    sel = torch.randn(6, 12, ODIM)
    models = {"dev": _device(base), "t32": copy.deepcopy(base).cuda(), "t64": copy.deepcopy(base).double().cuda()}
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
        print(f"cnn_tcn: {n}: float32 torch path {e_ref[n]:.3g} units from float64 -> bound {bound:.3g}; device path {e_dev[n]:.3g}")
        worst = max(worst, e_dev[n] / bound if bound > 0 else float(e_dev[n] > 0))
    error_report["dense_train_step/cnn_tcn/worst_fraction_of_bound"] = worst
    for n in names:
        assert e_dev[n] <= _bound(e_ref[n]), (n, e_dev[n], e_ref[n])


def test_three_training_steps(error_report):
    """Three TrainExecutor steps with ClipAdam from one initialisation, the rule of tests/test_hip_pointwise_train_step.py: the
    distance between the run with the swaps on and the float32 torch path is at most pow2_at_or_above(4 x the float32 torch
    path's distance from the float64 run), in units of 2^-24 (|p0| + |p64 - p0|).  Measured on MI355X: 1,930 units from the torch
    path, which is 1,700 from float64 (bound 8,192)."""
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(7)
    base = _base()
    loader = _loader((6, 8, 5), 12, 61)
    start = [p.detach().clone() for p in base.parameters()]
    m_dev, m_t32, m_t64 = _device(base), copy.deepcopy(base).cuda(), _Float64(copy.deepcopy(base)).cuda()
    TrainExecutor().train(m_dev, ClipAdam(m_dev.parameters(), **HYPER), loader, "cuda", None, ARGS)
    TrainExecutor().train(m_t32, ClipAdam(m_t32.parameters(), **HYPER), loader, "cuda", None, ARGS)
    TrainExecutor().train(m_t64, torch.optim.Adam(m_t64.parameters(), **HYPER), loader, "cuda", None, ARGS)
    p_dev, p_t32, p_t64 = (list(m.parameters()) for m in (m_dev, m_t32, m_t64))
    assert all(p.dtype == torch.float64 for p in p_t64)
    assert any(not torch.equal(p.cpu(), s) for p, s in zip(p_dev, start))
    d_ref = max(_distances(p_t32, p_t64, start, p_t64))
    d_dev = max(_distances(p_dev, p_t32, start, p_t64))
    bound = pow2_at_or_above(4 * d_ref)
    print(f"cnn_tcn: float32 torch path from float64: {d_ref:.3g} units -> bound {bound:.3g}; device path from torch's: {d_dev:.3g}")
    error_report["dense_train_step/cnn_tcn/torch32_from_float64"] = d_ref
    error_report["dense_train_step/cnn_tcn/device_from_torch32"] = d_dev
    assert d_dev <= bound, (d_dev, d_ref, bound)


def test_training_step_reads_nothing_on_the_host(monkeypatch):
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(8)
    model = _device(_base())
    start = [p.detach().clone() for p in model.parameters()]
    loader = _loader((6, 8, 5), 12, 62)
    opt = ClipAdam(model.parameters(), **HYPER)                                   # the parameters become views of flat buffers
    TrainExecutor().train(model, opt, loader[:1], "cuda", None, ARGS)           # (the first call of a kernel loads its code object)
    torch.cuda.synchronize()
    with monkeypatch.context() as mp:
        counter = _Counter(mp)
        TrainExecutor().train(model, opt, loader, "cuda", None, ARGS)
        reads = list(counter.calls)
    assert reads == [], reads
    assert int(opt.steps) == 1 + len(loader) and int(opt.skipped_steps) == 0
    assert any(not torch.equal(p, s) for p, s in zip(model.parameters(), start))


def test_trained_state_dict_is_served_by_the_packed_model():
    """train -> pack -> serve: the state dict of the model trained with the swaps on loads into init_model's packed KWSModel
    (type: tcn, ds: false), whose posteriors agree with the module's in eval() at the bar of tests/test_hip_parity.py."""
    from wekws_amd.model.kws_model import init_model
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(9)
    base = _base()
    keys = list(base.state_dict())
    model = _device(base)
    assert list(model.state_dict()) == keys
    TrainExecutor().train(model, ClipAdam(model.parameters(), **HYPER), _loader((6, 8, 5), 12, 63), "cuda", None, ARGS)
    cfg = dict(input_dim=IDIM, output_dim=ODIM, hidden_dim=HDIM, preprocessing=dict(type="linear"), backbone=BACKBONE_CFG)
    packed = init_model(cfg)
    packed.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    packed = packed.cuda().eval()
    x = torch.randn(4, 30, IDIM, device="cuda")
    model.eval()
    with torch.no_grad():
        want, cache = model(x)
    y, pc = packed(x)
    err, cerr = float((y - want).abs().max()), float((pc - cache).abs().max())
    print(f"cnn_tcn: packed posteriors vs the trained module: max|err| = {err:.2e} (bar {tol_for(want.cpu().numpy()):.1e}), cache {cerr:.2e}")
    assert y.shape == want.shape and err <= tol_for(want.cpu().numpy())
    assert pc.shape == cache.shape and cerr <= tol_for(cache.cpu().numpy())
