"""CPU: wekws_amd.model.pointwise without a device -- the swap's counts on this package's mirrors and on the reference's recorded
state-dict layouts, sharing and idempotence, state-dict keys, the order of the use_device_* swaps, what is left alone, and CPU and
float64 tensors through PointwiseConv1d equal to nn.Conv1d's bits."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from wekws_amd.model import batchnorm, depthwise, mdtc, pointwise, tcn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODELS = {
    "tcn_ds": (lambda: tcn.TCN(4, 64, 8, block_class=tcn.DsCnnBlock), 4),
    "mdtc_recipe": (lambda: mdtc.MDTC(3, 4, 32, 32, 5, True), 26),
    "mdtc_small": (lambda: mdtc.MDTC(3, 4, 80, 32, 5, True), 26),
    "tcn_tiny_cnn": (lambda: tcn.TCN(2, 8, 3, block_class=tcn.CnnBlock), 0),
    "tcn_tiny_ds": (lambda: tcn.TCN(2, 8, 3, block_class=tcn.DsCnnBlock), 2),
    "mdtc_tiny_sq": (lambda: mdtc.MDTC(2, 2, 8, 8, 3, True), 10),
}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "depthwise_conv_golden.npz"))


@pytest.mark.parametrize("tag", sorted(MODELS))
def test_swap_counts_sharing_and_idempotence(golden, tag):
    make, count = MODELS[tag]
    model = make()
    params, keys = list(model.parameters()), list(model.state_dict())
    convs = {n: m for n, m in model.named_modules() if type(m) is nn.Conv1d and m.kernel_size == (1,)}
    assert pointwise.use_device_pointwise_convs(model) == count == len(convs)
    swapped = {n: m for n, m in model.named_modules() if type(m) is pointwise.PointwiseConv1d}
    assert set(swapped) == set(convs)
    for n, m in swapped.items():
        assert m.weight is convs[n].weight and m.bias is convs[n].bias and m.training == convs[n].training
        assert (m.in_channels, m.out_channels, m.kernel_size) == (convs[n].in_channels, convs[n].out_channels, (1,))
    after = list(model.parameters())
    assert len(after) == len(params) and all(a is b for a, b in zip(after, params))      # the very objects an optimiser holds
    assert list(model.state_dict()) == keys
    assert pointwise.use_device_pointwise_convs(model) == 0
    if f"{tag}/keys" in golden.files:
        # the reference's own layout: as many (Co, Ci, 1) weights with Ci > 1 as convolutions swapped, under the same keys
        ref_keys = [str(k) for k in golden[f"{tag}/keys"]]
        assert keys == ref_keys
        shapes = [tuple(int(d) for d in str(s).split(",")) if str(s) else () for s in golden[f"{tag}/shapes"]]
        ones = [k for k, s in zip(ref_keys, shapes) if len(s) == 3 and s[2] == 1 and s[1] > 1]
        assert len(ones) == count and sorted(ones) == sorted(n + ".weight" for n in swapped)


def test_the_swaps_commute():
    """Every order of the three swaps gives the same module types, keys and parameter objects."""
    def types(order):
        torch.manual_seed(3)
        model = mdtc.MDTC(2, 2, 8, 8, 3, True)
        params = list(model.parameters())
        counts = {f.__name__: f(model) for f in order}
        assert all(a is b for a, b in zip(model.parameters(), params))
        return [type(m).__name__ for m in model.modules()], list(model.state_dict()), counts

    swaps = (pointwise.use_device_pointwise_convs, depthwise.use_device_depthwise_convs, batchnorm.use_device_batchnorms)
    first = types(swaps)
    assert first[2]["use_device_pointwise_convs"] == 10
    for order in ((swaps[2], swaps[0], swaps[1]), (swaps[1], swaps[2], swaps[0])):
        assert types(order) == first


def test_swap_leaves_everything_else_alone():
    class Mine(nn.Conv1d):
        pass

    net = nn.Sequential(nn.Conv1d(6, 8, 1), nn.Conv1d(6, 6, 1, stride=2), nn.Conv1d(6, 6, 1, padding=1), nn.Conv1d(6, 6, 1, groups=2),
                        nn.Conv1d(6, 6, 3), nn.Conv1d(6, 6, 1, padding_mode="replicate"), nn.Conv2d(6, 6, 1), Mine(6, 6, 1),
                        depthwise.DepthwiseConv1d(6, 6, 1, groups=6), pointwise.PointwiseConv1d(6, 6, 1), nn.Linear(6, 6),
                        nn.Sequential(nn.Conv1d(4, 5, 1, bias=False)))
    net[0].eval()
    before = list(net)
    assert pointwise.use_device_pointwise_convs(net) == 2
    assert type(net[0]) is pointwise.PointwiseConv1d and type(net[11][0]) is pointwise.PointwiseConv1d and net[11][0].bias is None
    assert all(net[i] is before[i] for i in range(1, 11))
    assert net[0].weight is before[0].weight and net[0].bias is before[0].bias and not net[0].training


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_and_float64_tensors_are_nn_conv1ds_bits(bias, dtype):
    torch.manual_seed(11)
    ref = nn.Conv1d(6, 9, 1, bias=bias).to(dtype)
    dev = pointwise.PointwiseConv1d.sharing(ref)
    x = torch.randn(3, 6, 17, dtype=dtype)
    sel = torch.randn(3, 9, 17, dtype=dtype)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya = ref(xa)
    ya.backward(sel)
    grads = [p.grad.clone() for p in ref.parameters()]
    ref.zero_grad()
    yb = dev(xb)
    yb.backward(sel)
    assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    assert all(torch.equal(a, p.grad) for a, p in zip(grads, dev.parameters()))
    # 2-D (unbatched) and non-contiguous inputs, and a convolution that is not pointwise, are nn.Conv1d's own too
    assert torch.equal(dev(x[0]), ref(x[0]))
    xt = torch.randn(3, 17, 6, dtype=dtype).transpose(1, 2)
    assert torch.equal(dev(xt), ref(xt))
    wide = pointwise.PointwiseConv1d(6, 9, 3, padding=1, bias=bias).to(dtype)
    assert torch.equal(wide(x), nn.functional.conv1d(x, wide.weight, wide.bias, padding=1))


def test_state_dicts_go_both_ways():
    torch.manual_seed(5)
    a, b = tcn.TCN(2, 8, 3, block_class=tcn.DsCnnBlock), tcn.TCN(2, 8, 3, block_class=tcn.DsCnnBlock)
    pointwise.use_device_pointwise_convs(a)
    b.load_state_dict(a.state_dict())
    a.load_state_dict(b.state_dict())
    x = torch.randn(2, 9, 8)
    a.eval(), b.eval()
    with torch.no_grad():
        assert torch.equal(a(x)[0], b(x)[0])
