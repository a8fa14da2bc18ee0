"""CPU: wekws_amd.model.dense without a device -- the swap's counts on this package's mirrors and on the reference's recorded
state-dict layouts, sharing and idempotence, state-dict keys, the order of the use_device_* swaps, what is left alone, and CPU and
float64 tensors through DenseConv1d and a swapped CnnBlock equal to nn.Conv1d's bits."""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from wekws_amd.model import batchnorm, dense, depthwise, mdtc, pointwise, tcn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Subsampling1(nn.Module):
    """The reference's Conv1dSubsampling1 (wekws/model/subsampling.py), layer for layer."""

    def __init__(self, idim, odim):
        super().__init__()
        self.out = nn.Sequential(nn.Conv1d(idim, odim, 3), nn.BatchNorm1d(odim), nn.ReLU())


MODELS = {
    "tcn_cnn": (lambda: tcn.TCN(4, 64, 8, block_class=tcn.CnnBlock), 4),
    "tcn_ds": (lambda: tcn.TCN(4, 64, 8, block_class=tcn.DsCnnBlock), 0),
    "mdtc_recipe": (lambda: mdtc.MDTC(3, 4, 32, 32, 5, True), 0),
    "subsampling1": (lambda: Subsampling1(40, 64), 1),
    "tcn_tiny_cnn": (lambda: tcn.TCN(2, 8, 3, block_class=tcn.CnnBlock), 2),
}


def _is_dense(m):
    return type(m) is nn.Conv1d and m.groups == 1 and m.kernel_size[0] >= 2


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "dense_conv_golden.npz"))


@pytest.mark.parametrize("tag", sorted(MODELS))
def test_swap_counts_sharing_and_idempotence(golden, tag):
    make, count = MODELS[tag]
    model = make()
    params, keys = list(model.parameters()), list(model.state_dict())
    convs = {n: m for n, m in model.named_modules() if _is_dense(m)}
    assert dense.use_device_dense_convs(model) == count == len(convs)
    swapped = {n: m for n, m in model.named_modules() if type(m) is dense.DenseConv1d}
    assert set(swapped) == set(convs)
    for n, m in swapped.items():
        assert m.weight is convs[n].weight and m.bias is convs[n].bias and m.training == convs[n].training
        assert (m.in_channels, m.out_channels, m.kernel_size, m.dilation) == (convs[n].in_channels, convs[n].out_channels,
                                                                              convs[n].kernel_size, convs[n].dilation)
    after = list(model.parameters())
    assert len(after) == len(params) and all(a is b for a, b in zip(after, params))      # the very objects an optimiser holds
    assert list(model.state_dict()) == keys
    assert dense.use_device_dense_convs(model) == 0
    if f"{tag}/keys" in golden.files:
        # the reference's own layout: as many (Co, Ci, K >= 2) weights with Ci > 1 as convolutions swapped, under the same keys
        ref_keys = [str(k) for k in golden[f"{tag}/keys"]]
        assert keys == ref_keys
        shapes = [tuple(int(d) for d in str(s).split(",")) if str(s) else () for s in golden[f"{tag}/shapes"]]
        assert shapes == [tuple(v.shape) for v in model.state_dict().values()]
        wide = [k for k, s in zip(ref_keys, shapes) if len(s) == 3 and s[2] >= 2 and s[1] > 1]
        assert len(wide) == count and sorted(wide) == sorted(n + ".weight" for n in swapped)


def test_the_recorded_layouts_are_there(golden):
    assert "tcn_cnn/keys" in golden.files and "subsampling1/keys" in golden.files


def test_the_swaps_commute():
    """Every order of the four swaps gives the same module types, keys and parameter objects, on a model that holds dense,
    depthwise and pointwise convolutions and BatchNorms."""
    def types(order):
        torch.manual_seed(3)
        model = nn.ModuleDict(dict(cnn=tcn.TCN(2, 8, 3, block_class=tcn.CnnBlock), ds=tcn.TCN(2, 8, 3, block_class=tcn.DsCnnBlock),
                                   mdtc=mdtc.MDTC(2, 2, 8, 8, 3, True), sub=Subsampling1(5, 8)))
        params = list(model.parameters())
        counts = {f.__name__: f(model) for f in order}
        assert all(a is b for a, b in zip(model.parameters(), params))
        return [type(m).__name__ for m in model.modules()], list(model.state_dict()), counts

    swaps = (dense.use_device_dense_convs, pointwise.use_device_pointwise_convs, depthwise.use_device_depthwise_convs,
             batchnorm.use_device_batchnorms)
    first = types(swaps)
    assert first[2]["use_device_dense_convs"] == 3 and first[2]["use_device_pointwise_convs"] == 12
    for order in itertools.permutations(swaps):
        assert types(order) == first


def test_swap_leaves_everything_else_alone():
    class Mine(nn.Conv1d):
        pass

    net = nn.Sequential(nn.Conv1d(6, 8, 3, dilation=2), nn.Conv1d(6, 6, 3, stride=2), nn.Conv1d(6, 6, 3, padding=1),
                        nn.Conv1d(6, 6, 3, groups=2), nn.Conv1d(6, 6, 1), nn.Conv1d(6, 6, 3, padding_mode="replicate"), nn.Conv2d(6, 6, 3),
                        Mine(6, 6, 3), depthwise.DepthwiseConv1d(6, 6, 3, groups=6), dense.DenseConv1d(6, 6, 3), nn.Linear(6, 6),
                        nn.Conv1d(6, 6, 33), nn.Conv1d(6, 6, 2, dilation=256), nn.Conv1d(6, 6, 3, groups=6),
                        nn.Sequential(nn.Conv1d(4, 5, 32, dilation=8, bias=False)))
    net[0].eval()
    before = list(net)
    assert dense.use_device_dense_convs(net) == 2
    assert type(net[0]) is dense.DenseConv1d and type(net[14][0]) is dense.DenseConv1d and net[14][0].bias is None
    assert all(net[i] is before[i] for i in range(1, 14))
    assert net[0].weight is before[0].weight and net[0].bias is before[0].bias and not net[0].training
    assert net[0].dilation == (2,) and net[14][0].dilation == (8,)
    # disjoint from the pointwise swap's predicate
    assert pointwise.use_device_pointwise_convs(net) == 1 and type(net[4]) is pointwise.PointwiseConv1d


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_and_float64_tensors_are_nn_conv1ds_bits(bias, dtype):
    torch.manual_seed(11)
    ref = nn.Conv1d(6, 9, 3, dilation=2, bias=bias).to(dtype)
    dev = dense.DenseConv1d.sharing(ref)
    x = torch.randn(3, 6, 17, dtype=dtype)
    for left_pad in (0, 3, 4):
        sel = torch.randn(3, 9, 17 + left_pad - 4, dtype=dtype)
        xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
        ya = ref(F.pad(xa, (left_pad, 0), value=0.0))
        ya.backward(sel)
        grads = [p.grad.clone() for p in ref.parameters()]
        ref.zero_grad()
        yb = dev(xb, left_pad)
        yb.backward(sel)
        assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
        assert all(torch.equal(a, p.grad) for a, p in zip(grads, dev.parameters()))
        dev.zero_grad()
    # 2-D (unbatched) and non-contiguous inputs, and a convolution that is not eligible, are nn.Conv1d's own too
    assert torch.equal(dev(x[0]), ref(x[0]))
    xt = torch.randn(3, 17, 6, dtype=dtype).transpose(1, 2)
    assert torch.equal(dev(xt), ref(xt))
    strided = dense.DenseConv1d(6, 9, 3, stride=2, padding=1, bias=bias).to(dtype)
    assert torch.equal(strided(x), F.conv1d(x, strided.weight, strided.bias, stride=2, padding=1))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_a_swapped_cnn_block_on_the_cpu_is_the_unswapped_ones_bits(dtype):
    torch.manual_seed(13)
    ref = tcn.TCN(2, 8, 3, dropout=0.0, block_class=tcn.CnnBlock).to(dtype)
    dev = tcn.TCN(2, 8, 3, dropout=0.0, block_class=tcn.CnnBlock).to(dtype)
    dev.load_state_dict(ref.state_dict())
    assert dense.use_device_dense_convs(dev) == 2
    x = torch.randn(3, 11, 8, dtype=dtype)
    for mode in ("train", "eval"):
        getattr(ref, mode)(), getattr(dev, mode)()
        xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
        (ya, ca), (yb, cb) = ref(xa), dev(xb)
        ya.sum().backward(), yb.sum().backward()
        assert torch.equal(ya, yb) and torch.equal(ca, cb) and torch.equal(xa.grad, xb.grad)
        assert all(torch.equal(p.grad, q.grad) for p, q in zip(ref.parameters(), dev.parameters()))
        ref.zero_grad(), dev.zero_grad()
    with torch.no_grad():                                                # streaming: the carried cache
        (y1, c1), (z1, d1) = ref(x[:, :4]), dev(x[:, :4])
        (y2, c2), (z2, d2) = ref(x[:, 4:], c1), dev(x[:, 4:], d1)
    assert torch.equal(y1, z1) and torch.equal(y2, z2) and torch.equal(c2, d2)


def test_state_dicts_go_both_ways():
    torch.manual_seed(5)
    a, b = tcn.TCN(2, 8, 3, block_class=tcn.CnnBlock), tcn.TCN(2, 8, 3, block_class=tcn.CnnBlock)
    dense.use_device_dense_convs(a)
    b.load_state_dict(a.state_dict())
    a.load_state_dict(b.state_dict())
    x = torch.randn(2, 9, 8)
    a.eval(), b.eval()
    with torch.no_grad():
        assert torch.equal(a(x)[0], b(x)[0])
