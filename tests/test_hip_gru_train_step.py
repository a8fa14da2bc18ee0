"""GPU: training a tiny GRU keyword model (hidden 16, 2 layers, linear preprocessing, max_pooling) with ``use_device_grus``: one
forward / backward against a float64 run, three ``TrainExecutor`` steps with ``ClipAdam`` against the same model with torch's
``nn.GRU``, no host read in the step, and the trained state dict served by the packed inference model."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.helpers import pow2_at_or_above, tol_for
from tests.train_step import ARGS, HYPER, _Counter, _distances, _Float64, _loader
from wekws_amd.model import gru as dg

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
IDIM, HDIM, ODIM, LAYERS = 20, 16, 2, 2                  # (IDIM and ODIM are those of test_hip_conv_train's _loader)


class _Prep(nn.Module):
    def __init__(self):
        super().__init__()
        self.out = nn.Sequential(nn.Linear(IDIM, HDIM), nn.ReLU())


class _Head(nn.Module):
    def __init__(self):
        super().__init__()
        self.linear = nn.Linear(HDIM, ODIM)


class Kws(nn.Module):
    """The reference's KWSModel for the gru recipe, as far as training goes, under the reference's state-dict keys.  As the
    reference does, it hands the backbone an empty cache when it is given none."""

    def __init__(self):
        super().__init__()
        self.preprocessing, self.backbone, self.classifier = _Prep(), nn.GRU(HDIM, HDIM, num_layers=LAYERS, batch_first=True), _Head()

    def forward(self, x, cache=None):
        if cache is None:
            cache = torch.zeros(0, 0, 0, dtype=x.dtype, device=x.device)
        if cache.numel() == 0 and not isinstance(self.backbone, dg.DeviceGRU):
            cache = None                                 # torch's nn.GRU refuses the reference's empty cache: zeros by omission
        y, cache = self.backbone(self.preprocessing.out(x), cache)
        return torch.sigmoid(self.classifier.linear(y)), cache


def _grad_errors(model, ref):
    out = {}
    pr = dict(ref.named_parameters())
    for n, p in model.named_parameters():
        a, r = p.grad.detach().double().cpu().numpy(), pr[n].grad.detach().double().cpu().numpy()
        scale = U * np.abs(r).max()
        assert np.isfinite(a).all() and scale > 0, n
        out[n] = float(np.abs(a - r).max() / scale)
    return out


def test_one_forward_backward_against_float64(error_report):
    """For every parameter tensor the gradient error of the model with device GRUs against the float64 run is at most
    pow2_at_or_above(4 x the float32 torch path's)."""
    torch.manual_seed(11)
    base = Kws()
    x, sel = torch.randn(6, 12, IDIM), torch.randn(6, 12, ODIM)
    models = {"dev": copy.deepcopy(base).cuda(), "t32": copy.deepcopy(base).cuda(), "t64": copy.deepcopy(base).double().cuda()}
    assert dg.use_device_grus(models["dev"]) == 1 and isinstance(models["dev"].backbone, dg.DeviceGRU)
    assert type(models["t32"].backbone) is nn.GRU
    for tag, m in models.items():
        m.train()
        dt = torch.float64 if tag == "t64" else torch.float32
        y, cache = m(x.to("cuda", dt))
        assert cache.shape == (LAYERS, 6, HDIM)
        (y * sel.to("cuda", dt)).sum().backward()
    e_ref, e_dev = _grad_errors(models["t32"], models["t64"]), _grad_errors(models["dev"], models["t64"])
    for n in e_ref:
        bound = pow2_at_or_above(4 * e_ref[n]) if e_ref[n] > 0 else 0.0
        print(f"{n}: float32 torch path {e_ref[n]:.3g} units from float64 -> bound {bound:.3g}; device GRU {e_dev[n]:.3g}")
        error_report[f"gru_train_step/{n}"] = e_dev[n]
    for n in e_ref:
        assert e_dev[n] <= (pow2_at_or_above(4 * e_ref[n]) if e_ref[n] > 0 else 0.0), (n, e_dev[n], e_ref[n])


def test_three_training_steps_with_device_grus_and_with_torch_grus(error_report):
    """Three TrainExecutor steps (max_pooling criterion, ClipAdam) from one initialisation, the rule of
    tests/test_hip_conv_train.py: the distance between the run with device GRUs and the float32 run with torch's is at most
    pow2_at_or_above(4 x the float32 torch path's distance from the float64 run), in units of 2^-24 (|p0| + |p64 - p0|)."""
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(7)
    base = Kws()
    loader = _loader((6, 8, 5), 12, 41)
    start = [p.detach().clone() for p in base.parameters()]
    m_dev = copy.deepcopy(base).cuda()
    assert dg.use_device_grus(m_dev) == 1
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
    print(f"float32 torch path from float64: {d_ref:.3g} units -> bound {bound:.3g}; device GRUs from torch's: {d_dev:.3g} units")
    error_report["gru_train_step/torch32_from_float64"] = d_ref
    error_report["gru_train_step/device_from_torch32"] = d_dev
    assert d_dev <= bound, (d_dev, d_ref, bound)


def test_training_step_reads_nothing_on_the_host(monkeypatch):
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(8)
    model = Kws().cuda()
    assert dg.use_device_grus(model) == 1
    start = [p.detach().clone() for p in model.parameters()]
    loader = _loader((6, 8, 5), 12, 42)
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
    """train -> pack -> serve: the state dict of the model trained with device GRUs loads into init_model's packed KWSModel, whose
    posteriors agree with the module's in eval() at the bar of tests/test_hip_parity.py."""
    from wekws_amd.model.kws_model import init_model
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(9)
    model = Kws().cuda()
    keys = list(model.state_dict())
    assert dg.use_device_grus(model) == 1 and list(model.state_dict()) == keys
    before = copy.deepcopy(model.state_dict())
    TrainExecutor().train(model, ClipAdam(model.parameters(), **HYPER), _loader((6, 8, 5), 12, 43), "cuda", None, ARGS)
    assert any(not torch.equal(v, before[k]) for k, v in model.state_dict().items() if k.startswith("backbone."))
    cfg = dict(input_dim=IDIM, output_dim=ODIM, hidden_dim=HDIM, preprocessing=dict(type="linear"),
               backbone=dict(type="gru", num_layers=LAYERS))
    packed = init_model(cfg)
    packed.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    packed = packed.cuda().eval()
    x = torch.randn(4, 30, IDIM, device="cuda")
    model.eval()
    with torch.no_grad():
        want, cache = model(x)
    y, pc = packed(x)
    err, cerr = float((y - want).abs().max()), float((pc - cache).abs().max())
    print(f"packed posteriors vs the trained module: max|err| = {err:.2e} (bar {tol_for(want.cpu().numpy()):.1e}), cache {cerr:.2e}")
    assert y.shape == want.shape and err <= tol_for(want.cpu().numpy())
    assert pc.shape == cache.shape and cerr <= tol_for(cache.cpu().numpy())
