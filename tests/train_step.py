"""The set-up the training-step tests share (test_hip_conv_train, test_hip_batchnorm_train, test_hip_gru_train_step,
test_hip_linear_train_step, test_hip_pointwise_train_step, test_hip_fsmn_train, test_hip_optim): the tiny keyword model and its
two backbones, the max_pooling loader, the float64 twin, the distances and bounds the runs are held to, the optimiser's
hyperparameters and the host-read counter.  It holds no tests."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.helpers import pow2_at_or_above
from wekws_amd.model import depthwise, mdtc, tcn

U = 2.0 ** -24
IDIM, HDIM, ODIM = 20, 8, 2
BACKBONES = {
    "ds_tcn": (lambda: tcn.TCN(2, HDIM, 3, dropout=0.0, block_class=tcn.DsCnnBlock),
               dict(type="tcn", ds=True, num_layers=2, kernel_size=3, dropout=0.0)),
    # (the tiny MDTC is square -- the reference's MDTC.forward concatenates caches of in_channels and of res_channels, so it
    # runs only where the two are equal, as init_model builds it)
    "mdtc": (lambda: mdtc.MDTC(2, 2, HDIM, HDIM, 3, True),
             dict(type="mdtc", num_stack=2, stack_size=2, kernel_size=3, hidden_dim=HDIM, causal=True)),
}


class TorchConv1d(nn.Conv1d):
    """A depthwise convolution that is not the package's: the parameters of ``conv`` under torch's own statement, whatever the
    device.  use_device_depthwise_convs sees an nn.Conv1d like any other."""

    def __init__(self, conv):
        super().__init__(conv.in_channels, conv.out_channels, conv.kernel_size[0], dilation=conv.dilation[0], groups=conv.groups,
                         bias=conv.bias is not None)
        self.weight, self.bias = conv.weight, conv.bias

    def forward(self, x, left_pad=0):
        return super().forward(F.pad(x, (left_pad, 0), value=0.0))


def torch_convs(model):
    """Every DepthwiseConv1d of ``model`` replaced by a TorchConv1d over the same parameters."""
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, depthwise.DepthwiseConv1d):
                setattr(parent, name, TorchConv1d(child))
    return model


class _Prep(nn.Module):
    def __init__(self):
        super().__init__()
        self.out = nn.Sequential(nn.Linear(IDIM, HDIM), nn.ReLU())


class _Head(nn.Module):
    def __init__(self):
        super().__init__()
        self.linear = nn.Linear(HDIM, ODIM)


class Kws(nn.Module):
    """The reference's KWSModel for a keyword recipe, as far as training goes: a Linear + ReLU in front of the backbone, a Linear
    classifier and a sigmoid behind it, under the reference's state-dict keys."""

    def __init__(self, backbone):
        super().__init__()
        self.preprocessing, self.backbone, self.classifier = _Prep(), backbone, _Head()

    def forward(self, x, cache=None):
        y, cache = self.backbone(self.preprocessing.out(x), cache)
        return torch.sigmoid(self.classifier.linear(y)), cache


def _loader(sizes, T, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(sizes):
        feats = rng.standard_normal((n, T, IDIM)).astype(np.float32)
        lengths = rng.integers(T // 2, T + 1, n).astype(np.int32)
        lengths[0] = T
        target = rng.integers(-1, ODIM, (n, 1)).astype(np.int64)
        out.append(dict(keys=[f"utt{i}_{j}" for j in range(n)], feats=torch.from_numpy(feats), target=torch.from_numpy(target),
                        feats_lengths=torch.from_numpy(lengths), target_lengths=torch.ones(n, dtype=torch.int32)))
    return out


class _Float64(nn.Module):
    """A float64 model behind the float32 interface of the device criterion."""

    def __init__(self, model):
        super().__init__()
        self.model = model.double()

    def forward(self, x):
        y, c = self.model(x.double())
        return y.float(), c


ARGS = {"criterion": "max_pooling", "grad_clip": 5.0, "log_interval": 100}


def _distances(a, b, start, ref):
    """Per parameter tensor, the worst |a - b| in units of U (|start| + |ref - start|): the scale of tests/optim_matrix.py's p'."""
    out = []
    for pa, pb, ps, pr in zip(a, b, start, ref):
        pa, pb, ps, pr = (t.detach().double().cpu().numpy() for t in (pa, pb, ps, pr))
        den = U * (np.abs(ps) + np.abs(pr - ps))
        err = np.abs(pa - pb)
        assert np.isfinite(err).all() and not np.any(err[den == 0])
        out.append(float((err[den > 0] / den[den > 0]).max()) if (den > 0).any() else 0.0)
    return out


SWAPPED = {"ds_tcn": 4, "mdtc": 15}                # BatchNorms of the tiny backbones: 2 a DsCnnBlock, 3 a TCNBlock


def _grad_errors(model, ref, names):
    """Per tensor of `names` (parameters' gradients, then buffers), the worst |a - ref| in units of U max|ref|; a reference
    that is all zeros demands zeros (inf otherwise)."""
    out = {}
    pa, pr = dict(model.named_parameters()), dict(ref.named_parameters())
    ba, brf = dict(model.named_buffers()), dict(ref.named_buffers())
    for n in names:
        a, r = (pa[n].grad, pr[n].grad) if n in pa else (ba[n], brf[n])
        a, r = a.detach().double().cpu().numpy(), r.detach().double().cpu().numpy()
        scale = U * np.abs(r).max()
        assert np.isfinite(a).all(), n
        out[n] = float(np.abs(a - r).max() / scale) if scale > 0 else (float("inf") if np.any(a) else 0.0)
    return out


def _bound(ref_units):
    return pow2_at_or_above(4 * ref_units) if 0 < ref_units < float("inf") else ref_units


HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)


class _Counter:
    def __init__(self, monkeypatch):
        self.calls = []
        for owner, name in ((torch.cuda, "synchronize"), (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "__bool__"),
                            (torch.Tensor, "__float__"), (torch.Tensor, "__int__"), (torch.Tensor, "cpu"), (torch.Tensor, "numpy")):
            monkeypatch.setattr(owner, name, self._wrap(getattr(owner, name), name))

    def _wrap(self, fn, name):
        def counted(*a, **k):
            self.calls.append(name)
            return fn(*a, **k)
        return counted
