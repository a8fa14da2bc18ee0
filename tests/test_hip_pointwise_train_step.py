"""GPU: a tiny DS-TCN and a tiny square MDTC (dropout 0) with ``use_device_depthwise_convs``, ``use_device_batchnorms`` and
``use_device_pointwise_convs`` all on, under the set-up and the rule of tests/test_hip_conv_train.py: one forward / backward per
parameter and three ``TrainExecutor`` steps (max_pooling, ClipAdam) against the float32 torch path and a float64 run, no host read
in the step, the trained state dict served by the packed inference model, and a module that was not swapped giving the bits of a
process that never imported wekws_amd.model.pointwise."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import pow2_at_or_above, tol_for
from tests.train_step import SWAPPED as BN_SWAPPED
from tests.train_step import (ARGS, BACKBONES, HDIM, HYPER, IDIM, ODIM, Kws, _bound, _Counter, _distances, _Float64, _grad_errors, _loader,
                              torch_convs)
from wekws_amd.model import batchnorm, depthwise, pointwise

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTWISE = {"ds_tcn": 2, "mdtc": 10}             # one a DsCnnBlock, two a TCNBlock (the preprocessor's and 2 x 2 stacked)
DEPTHWISE = {"ds_tcn": 2, "mdtc": 5}


def _device(base):
    """A copy of ``base`` (torch's convolutions and BatchNorms) on the device with the three swaps on."""
    m = copy.deepcopy(base).cuda()
    kind = "ds_tcn" if type(m.backbone).__name__ == "TCN" else "mdtc"
    assert pointwise.use_device_pointwise_convs(m) == POINTWISE[kind]
    assert depthwise.use_device_depthwise_convs(m) == DEPTHWISE[kind]
    assert batchnorm.use_device_batchnorms(m) == BN_SWAPPED[kind]
    assert sum(type(c) is pointwise.PointwiseConv1d for c in m.modules()) == POINTWISE[kind]
    return m


@pytest.mark.parametrize("kind", sorted(BACKBONES))
def test_one_forward_backward_against_float64(kind, error_report):
    """One forward / backward in train() from one initialisation: with the three swaps on, with torch's modules in float32 and
    with torch's in float64.  For every parameter tensor the device path's gradient error against the float64 run is at most
    pow2_at_or_above(4 x the float32 torch path's); the running buffers are held to the same rule.  Measured on MI355X, the
    tensor closest to its bound: ds_tcn classifier.linear.bias 5.25 units (torch path 1.67, bound 8); mdtc
    backbone.blocks.0.res_blocks.0.conv1.pointwise.bias 2.05e16 units (torch path 9.0e15, bound 3.6e16: a bias in front of a
    training-mode BatchNorm, whose exact gradient is zero -- both paths hold rounding noise, tests/test_hip_conv_train.py)."""
    torch.manual_seed(11)
    base = torch_convs(Kws(BACKBONES[kind][0]()))
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
        print(f"{kind}: {n}: float32 torch path {e_ref[n]:.3g} units from float64 -> bound {bound:.3g}; device path {e_dev[n]:.3g}")
        worst = max(worst, e_dev[n] / bound if bound > 0 else float(e_dev[n] > 0))
    error_report[f"pointwise_train_step/{kind}/worst_fraction_of_bound"] = worst
    for n in names:
        assert e_dev[n] <= _bound(e_ref[n]), (n, e_dev[n], e_ref[n])


@pytest.mark.parametrize("kind", sorted(BACKBONES))
def test_three_training_steps(kind, error_report):
    """Three TrainExecutor steps with ClipAdam from one initialisation, the rule of tests/test_hip_conv_train.py: the distance
    between the run with the three swaps on and the float32 torch path is at most pow2_at_or_above(4 x the float32 torch path's
    distance from the float64 run), in units of 2^-24 (|p0| + |p64 - p0|).  Measured on MI355X: ds_tcn 496 units from the torch path,
    which is 838 from float64 (bound 4096); mdtc 6.2e16 units, the torch path 5.0e16 (bound 2.9e17: the noise-driven biases in front
    of the BatchNorms, tests/test_hip_conv_train.py)."""
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(7)
    base = torch_convs(Kws(BACKBONES[kind][0]()))
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
    print(f"{kind}: float32 torch path from float64: {d_ref:.3g} units -> bound {bound:.3g}; device path from torch's: {d_dev:.3g}")
    error_report[f"pointwise_train_step/{kind}/torch32_from_float64"] = d_ref
    error_report[f"pointwise_train_step/{kind}/device_from_torch32"] = d_dev
    assert d_dev <= bound, (kind, d_dev, d_ref, bound)


@pytest.mark.parametrize("kind", sorted(BACKBONES))
def test_training_step_reads_nothing_on_the_host(kind, monkeypatch):
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(8)
    model = _device(torch_convs(Kws(BACKBONES[kind][0]())))
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


@pytest.mark.parametrize("kind", sorted(BACKBONES))
def test_trained_state_dict_is_served_by_the_packed_model(kind):
    """train -> pack -> serve: the state dict of the model trained with the three swaps on loads into init_model's packed
    KWSModel, whose posteriors agree with the module's in eval() at the bar of tests/test_hip_parity.py."""
    from wekws_amd.model.kws_model import init_model
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(9)
    make, bb_cfg = BACKBONES[kind]
    base = torch_convs(Kws(make()))
    keys = list(base.state_dict())
    model = _device(base)
    assert list(model.state_dict()) == keys
    TrainExecutor().train(model, ClipAdam(model.parameters(), **HYPER), _loader((6, 8, 5), 12, 63), "cuda", None, ARGS)
    cfg = dict(input_dim=IDIM, output_dim=ODIM, hidden_dim=HDIM, preprocessing=dict(type="linear"), backbone=bb_cfg)
    packed = init_model(cfg)
    packed.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    packed = packed.cuda().eval()
    x = torch.randn(4, 30, IDIM, device="cuda")
    model.eval()
    with torch.no_grad():
        want, cache = model(x)
    y, pc = packed(x)
    err, cerr = float((y - want).abs().max()), float((pc - cache).abs().max())
    print(f"{kind}: packed posteriors vs the trained module: max|err| = {err:.2e} (bar {tol_for(want.cpu().numpy()):.1e}), cache {cerr:.2e}")
    assert y.shape == want.shape and err <= tol_for(want.cpu().numpy())
    assert pc.shape == cache.shape and cerr <= tol_for(cache.cpu().numpy())


_CHILD = r"""
import sys
import numpy as np
import torch
from wekws_amd.model import mdtc
torch.manual_seed(21)
m = mdtc.TCNBlock(8, 8, 3, 2, True).cuda().train()
x = torch.randn(5, 8, 19, device="cuda", requires_grad=True)
sel = torch.randn(5, 8, 19, device="cuda")
y, cache = m(x)
(y * sel).sum().backward()
assert "wekws_amd.model.pointwise" not in sys.modules
np.savez(sys.argv[1], y=y.detach().cpu().numpy(), x=x.grad.cpu().numpy(),
         **{n.replace(".", "_"): p.grad.cpu().numpy() for n, p in m.named_parameters()})
"""


def test_a_module_that_was_not_swapped_is_the_code_that_never_saw_this_module(tmp_path):
    """Existing behaviour is unchanged: a TCNBlock that was not swapped, in this process where wekws_amd.model.pointwise is
    imported and has swapped another model, gives the bits of a fresh process that never imported it."""
    from wekws_amd.model import mdtc
    out = str(tmp_path / "grads.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-c", _CHILD, out], check=True, cwd=ROOT, env=env, timeout=300)
    want = np.load(out)
    other = mdtc.TCNBlock(8, 8, 3, 2, True).cuda()
    assert pointwise.use_device_pointwise_convs(other) == 2
    other(torch.randn(2, 8, 9, device="cuda"))[0].sum().backward()
    torch.manual_seed(21)
    m = mdtc.TCNBlock(8, 8, 3, 2, True).cuda().train()
    assert type(m.conv2) is torch.nn.Conv1d and type(m.conv1.pointwise) is torch.nn.Conv1d
    x = torch.randn(5, 8, 19, device="cuda", requires_grad=True)
    sel = torch.randn(5, 8, 19, device="cuda")
    y, _ = m(x)
    (y * sel).sum().backward()
    assert np.array_equal(y.detach().cpu().numpy().view(np.uint32), want["y"].view(np.uint32))
    assert np.array_equal(x.grad.cpu().numpy().view(np.uint32), want["x"].view(np.uint32))
    for n, p in m.named_parameters():
        assert np.array_equal(p.grad.cpu().numpy().view(np.uint32), want[n.replace(".", "_")].view(np.uint32)), n
