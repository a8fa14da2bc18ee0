"""GPU: training with ``use_device_weight_grads`` -- a tiny FSMN (device memory blocks too) and a tiny GRU keyword model
(``use_device_grus`` too): one forward / backward against a float64 run per parameter, three ``TrainExecutor`` steps with
``ClipAdam``, no host read in the step, the trained state dict served by the packed inference model, and DeviceGRU's gradients
with the switch off against a run made in a process that never imported wekws_amd.model.linear.

The shapes are those of tests/test_hip_fsmn_train.py and tests/test_hip_gru_train_step.py, whose rule this file applies:
pow2_at_or_above(4 x the float32 torch path's distance from the float64 run)."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import test_hip_fsmn_train as tf
from tests import test_hip_gru_train_step as tg
from tests.helpers import pow2_at_or_above, tol_for
from tests.train_step import ARGS as MAXPOOL_ARGS
from tests.train_step import HYPER, _Counter, _distances
from tests.train_step import _loader as maxpool_loader
from wekws_amd.model import fsmn
from wekws_amd.model import gru as dg
from wekws_amd.model import linear as dl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _variants(kind, base):
    """-> (device model, float32 torch-path model, float64 torch-path model), on the device, from one initialisation."""
    if kind == "fsmn":
        dev = copy.deepcopy(base).cuda()
        assert all(type(u[1]) is fsmn.FSMNBlock for u in dev.fsmn) and dl.use_device_weight_grads(dev) == 8
        return dev, tf.torch_blocks(copy.deepcopy(base)).cuda(), tf.torch_blocks(copy.deepcopy(base)).double().cuda()
    dev = copy.deepcopy(base).cuda()
    assert dg.use_device_grus(dev) == 1 and dl.use_device_weight_grads(dev) == 3 and dev.backbone.device_weight_grads
    assert type(dev.preprocessing.out[0]) is dl.DeviceLinear and type(dev.classifier.linear) is dl.DeviceLinear
    return dev, copy.deepcopy(base).cuda(), copy.deepcopy(base).double().cuda()


def _base(kind):
    return fsmn.FSMN(*tf.TINY) if kind == "fsmn" else tg.Kws()


def _setup(kind):
    """-> (loader, executor arguments)"""
    if kind == "fsmn":
        return tf._loader, tf.ARGS
    return maxpool_loader, MAXPOOL_ARGS


@pytest.mark.parametrize("kind", ["fsmn", "gru"])
def test_one_forward_backward_against_float64(kind, error_report):
    """For every parameter tensor the gradient error of the model with device weight gradients against the float64 run is at
    most pow2_at_or_above(4 x the float32 torch path's).  Measured on MI355X, the parameter closest to its bound: fsmn
    out_linear2.linear.bias 4.66 units (torch path 1.07, bound 8); gru backbone.bias_ih_l1 3.66 units (torch path 1.28, bound 8)."""
    torch.manual_seed(11)
    base = _base(kind)
    odim = 7 if kind == "fsmn" else tg.ODIM
    x, sel = torch.randn(6, 12, 20), torch.randn(6, 12, odim)
    dev, t32, t64 = _variants(kind, base)
    for m, dt in ((dev, torch.float32), (t32, torch.float32), (t64, torch.float64)):
        m.train()
        y, _ = m(x.to("cuda", dt))
        (y * sel.to("cuda", dt)).sum().backward()
    e_ref, e_dev = tg._grad_errors(t32, t64), tg._grad_errors(dev, t64)
    for n in e_ref:
        bound = pow2_at_or_above(4 * e_ref[n]) if e_ref[n] > 0 else 0.0
        print(f"{kind} {n}: float32 torch path {e_ref[n]:.3g} units from float64 -> bound {bound:.3g}; device weight gradients {e_dev[n]:.3g}")
        error_report[f"linear_train_step/{kind}/{n}"] = e_dev[n]
    for n in e_ref:
        assert e_dev[n] <= (pow2_at_or_above(4 * e_ref[n]) if e_ref[n] > 0 else 0.0), (kind, n, e_dev[n], e_ref[n])


@pytest.mark.parametrize("kind", ["fsmn", "gru"])
def test_three_training_steps(kind, error_report):
    """Three TrainExecutor steps with ClipAdam from one initialisation, the rule of tests/test_hip_conv_train.py: the distance
    between the run with device weight gradients and the float32 torch path is at most pow2_at_or_above(4 x the float32 torch
    path's distance from the float64 run), in units of 2^-24 (|p0| + |p64 - p0|).  Measured on MI355X: fsmn 3.30 units from the
    torch path, which is 3.45 from float64 (bound 16); gru 504 units, the torch path 173 (bound 1024)."""
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(7)
    base = _base(kind)
    make_loader, args = _setup(kind)
    loader = make_loader((6, 8, 5), 12, 51)
    start = [p.detach().clone() for p in base.parameters()]
    m_dev, m_t32, m_t64 = _variants(kind, base)
    m_t64 = tf._Float64(m_t64)
    TrainExecutor().train(m_dev, ClipAdam(m_dev.parameters(), **HYPER), loader, "cuda", None, args)
    TrainExecutor().train(m_t32, ClipAdam(m_t32.parameters(), **HYPER), loader, "cuda", None, args)
    TrainExecutor().train(m_t64, torch.optim.Adam(m_t64.parameters(), **HYPER), loader, "cuda", None, args)
    p_dev, p_t32, p_t64 = (list(m.parameters()) for m in (m_dev, m_t32, m_t64))
    assert all(p.dtype == torch.float64 for p in p_t64)
    assert any(not torch.equal(p.cpu(), s) for p, s in zip(p_dev, start))
    d_ref = max(_distances(p_t32, p_t64, start, p_t64))
    d_dev = max(_distances(p_dev, p_t32, start, p_t64))
    bound = pow2_at_or_above(4 * d_ref)
    print(f"{kind}: float32 torch path from float64: {d_ref:.3g} units -> bound {bound:.3g}; device weight gradients from torch's: {d_dev:.3g}")
    error_report[f"linear_train_step/{kind}/torch32_from_float64"] = d_ref
    error_report[f"linear_train_step/{kind}/device_from_torch32"] = d_dev
    assert d_dev <= bound, (kind, d_dev, d_ref, bound)


@pytest.mark.parametrize("kind", ["fsmn", "gru"])
def test_training_step_reads_nothing_on_the_host(kind, monkeypatch):
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(8)
    model, _, _ = _variants(kind, _base(kind))
    start = [p.detach().clone() for p in model.parameters()]
    make_loader, args = _setup(kind)
    loader = make_loader((6, 8, 5), 12, 52)
    opt = ClipAdam(model.parameters(), **HYPER)                                   # the parameters become views of flat buffers
    TrainExecutor().train(model, opt, loader[:1], "cuda", None, args)           # (the first call of a kernel loads its code object)
    torch.cuda.synchronize()
    with monkeypatch.context() as mp:
        counter = _Counter(mp)
        TrainExecutor().train(model, opt, loader, "cuda", None, args)
        reads = list(counter.calls)
    assert reads == [], reads
    assert int(opt.steps) == 1 + len(loader) and int(opt.skipped_steps) == 0
    assert any(not torch.equal(p, s) for p, s in zip(model.parameters(), start))


@pytest.mark.parametrize("kind", ["fsmn", "gru"])
def test_trained_state_dict_is_served_by_the_packed_model(kind):
    from wekws_amd.model.kws_model import init_model
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(9)
    base = _base(kind)
    keys = list(base.state_dict())
    model, _, _ = _variants(kind, base)
    assert list(model.state_dict()) == keys
    before = copy.deepcopy(model.state_dict())
    make_loader, args = _setup(kind)
    TrainExecutor().train(model, ClipAdam(model.parameters(), **HYPER), make_loader((6, 8, 5), 12, 53), "cuda", None, args)
    assert any(not torch.equal(v, before[k]) for k, v in model.state_dict().items())
    model.eval()
    x = torch.randn(4, 30, 20, device="cuda")
    if kind == "fsmn":
        packed = init_model(tf.TINY_CFG)
        packed.load_state_dict({"backbone." + k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
        packed = packed.cuda().eval()
        with torch.no_grad():
            want = torch.softmax(model(x)[0], dim=-1).cpu().numpy()
        y, _ = packed.forward_softmax(x)
        assert y.shape == want.shape and float(np.abs(y.cpu().numpy() - want).max()) <= tol_for(want)
        return
    cfg = dict(input_dim=tg.IDIM, output_dim=tg.ODIM, hidden_dim=tg.HDIM, preprocessing=dict(type="linear"),
               backbone=dict(type="gru", num_layers=tg.LAYERS))
    packed = init_model(cfg)
    packed.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    packed = packed.cuda().eval()
    with torch.no_grad():
        want, cache = model(x)
    y, pc = packed(x)
    assert y.shape == want.shape and float((y - want).abs().max()) <= tol_for(want.cpu().numpy())
    assert pc.shape == cache.shape and float((pc - cache).abs().max()) <= tol_for(cache.cpu().numpy())


_CHILD = r"""
import sys
import numpy as np
import torch
from wekws_amd.model import gru as dg
torch.manual_seed(21)
m = dg.DeviceGRU(20, 16, num_layers=2, batch_first=True).cuda()
x = torch.randn(5, 9, 20, device="cuda", requires_grad=True)
sel = torch.randn(5, 9, 16, device="cuda")
y, hn = m(x)
((y * sel).sum() + hn.sum()).backward()
assert "wekws_amd.model.linear" not in sys.modules
np.savez(sys.argv[1], x=x.grad.cpu().numpy(), **{n.replace(".", "_"): p.grad.cpu().numpy() for n, p in m.named_parameters()})
"""


def test_switch_off_is_the_code_that_never_saw_this_module(tmp_path):
    """Existing behaviour is unchanged: DeviceGRU with the switch off, in this process where wekws_amd.model.linear is imported
    and has swapped other models, gives the bits of a fresh process that never imported it."""
    out = str(tmp_path / "grads.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-c", _CHILD, out], check=True, cwd=ROOT, env=env, timeout=300)
    want = np.load(out)
    other = tg.Kws().cuda()
    assert dg.use_device_grus(other) == 1 and dl.use_device_weight_grads(other) == 3
    torch.manual_seed(21)
    m = dg.DeviceGRU(20, 16, num_layers=2, batch_first=True).cuda()
    assert m.device_weight_grads is False
    x = torch.randn(5, 9, 20, device="cuda", requires_grad=True)
    sel = torch.randn(5, 9, 16, device="cuda")
    y, hn = m(x)
    ((y * sel).sum() + hn.sum()).backward()
    assert np.array_equal(x.grad.cpu().numpy().view(np.uint32), want["x"].view(np.uint32))
    for n, p in m.named_parameters():
        assert np.array_equal(p.grad.cpu().numpy().view(np.uint32), want[n.replace(".", "_")].view(np.uint32)), n
    # and with the switch on the parameter gradients are the kernels': close, and not torch's bits
    on = dg.DeviceGRU.sharing(m)
    on.device_weight_grads = True
    m.zero_grad()
    x2 = x.detach().clone().requires_grad_()
    y2, hn2 = on(x2)
    ((y2 * sel).sum() + hn2.sum()).backward()
    assert float((y2 - y).abs().max()) <= 1e-6 and float((x2.grad - x.grad).abs().max()) <= 1e-5
    for n, p in m.named_parameters():
        ref = want[n.replace(".", "_")]
        assert float(np.abs(p.grad.cpu().numpy() - ref).max()) <= 1e-4 * max(1.0, float(np.abs(ref).max())), n
