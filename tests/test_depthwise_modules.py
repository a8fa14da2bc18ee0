"""CPU: wekws_amd.model.tcn / .mdtc / .depthwise without a device -- the mirrors' state-dict layout against the live reference's,
their torch path against the reference's goldens bit for bit (one shot and in two chunks with a carried cache), the convolution
swap, and the refusal of CPU tensors."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from wekws_amd.model import depthwise, mdtc, tcn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODELS = {
    "tcn_ds": lambda: tcn.TCN(4, 64, 8, block_class=tcn.DsCnnBlock),
    "tcn_tiny_ds": lambda: tcn.TCN(2, 8, 3, block_class=tcn.DsCnnBlock),
    "tcn_tiny_cnn": lambda: tcn.TCN(2, 8, 3, block_class=tcn.CnnBlock),
    "mdtc_small": lambda: mdtc.MDTC(3, 4, 80, 32, 5, True),
    "mdtc_tiny": lambda: mdtc.MDTC(2, 2, 6, 8, 3, True),
    "mdtc_tiny_sq": lambda: mdtc.MDTC(2, 2, 8, 8, 3, True),
}
# the tags with forward goldens.  (MDTC.forward concatenates the preprocessor's cache, of in_channels channels, with the
# stacks', of res_channels: the reference's runs only where the two are equal, so mdtc_small and mdtc_tiny are layouts only.)
FORWARD = ("tcn_tiny_ds", "tcn_tiny_cnn", "mdtc_tiny_sq")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "depthwise_conv_golden.npz"))


@pytest.mark.parametrize("tag", sorted(MODELS))
def test_state_dict_layout_is_the_references(golden, tag):
    sd = MODELS[tag]().state_dict()
    assert list(sd) == [str(k) for k in golden[f"{tag}/keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in golden[f"{tag}/shapes"]]


def test_the_layout_is_what_the_packed_model_reads():
    from wekws_amd import pack
    from wekws_amd.utils import synth
    for name, make in (("ds_tcn_h64", lambda: tcn.TCN(4, 64, 8, block_class=tcn.DsCnnBlock)),
                       ("mdtc_small", lambda: mdtc.MDTC(3, 4, 32, 32, 5, True))):
        spec = {k: s for k, s in pack.model_spec(synth.MODEL_CONFIGS[name]) if k.startswith("backbone.")}
        sd = make().state_dict()
        assert {"backbone." + k: tuple(v.shape) for k, v in sd.items()} == spec, name


def _bits(t):
    return t.detach().numpy().view(np.int32)


@pytest.mark.parametrize("tag", FORWARD)
def test_torch_path_equals_the_reference_bit_for_bit(golden, tag):
    model = MODELS[tag]().eval()
    prefix = f"{tag}/sd/"
    model.load_state_dict({k[len(prefix):]: torch.from_numpy(golden[k].copy()) for k in golden.files if k.startswith(prefix)})
    x = torch.from_numpy(golden[f"{tag}/x"].copy())
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            y, cache = model(x)
            y_none, _ = model(x, None)
            y1, cache1 = model(x[:, :5])
            y2, cache2 = model(x[:, 5:], cache1)
    finally:
        torch.set_num_threads(threads)
    for k, v in dict(y=y, cache=cache, y1=y1, cache1=cache1, y2=y2, cache2=cache2).items():
        assert v.shape == golden[f"{tag}/{k}"].shape and np.array_equal(_bits(v), golden[f"{tag}/{k}"].view(np.int32)), (tag, k)
    assert torch.equal(y_none, y) and cache.shape == (3, 8, model.padding)


def test_padded_tail_is_the_references_cache():
    x = torch.randn(2, 3, 5)
    for p in (0, 1, 4, 5, 6, 9):
        assert torch.equal(tcn.padded_tail(x, p), F.pad(x, (p, 0), value=0.0)[:, :, -p:]), p


@pytest.mark.parametrize("tag,count", [("tcn_ds", 4), ("mdtc_small", 13), ("tcn_tiny_cnn", 0)])
def test_swap_counts_on_modules_that_are_not_ours(golden, tag, count):
    """A plain-torch twin of the backbone (every DepthwiseConv1d turned back into its nn.Conv1d): the swap finds exactly the
    depthwise convolutions, shares the parameter objects and is idempotent."""
    model = MODELS[tag]()
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, depthwise.DepthwiseConv1d):
                plain = nn.Conv1d(child.in_channels, child.out_channels, child.kernel_size[0], dilation=child.dilation[0],
                                  groups=child.groups, bias=child.bias is not None)
                plain.weight, plain.bias = child.weight, child.bias
                setattr(parent, name, plain)
    assert not any(isinstance(m, depthwise.DepthwiseConv1d) for m in model.modules())
    params, keys = list(model.parameters()), list(model.state_dict())
    assert depthwise.use_device_depthwise_convs(model) == count
    assert sum(isinstance(m, depthwise.DepthwiseConv1d) for m in model.modules()) == count
    after = list(model.parameters())
    assert len(after) == len(params) and all(a is b for a, b in zip(after, params))      # the very objects an optimiser holds
    assert list(model.state_dict()) == keys == [str(k) for k in golden[f"{tag}/keys"]]
    assert depthwise.use_device_depthwise_convs(model) == 0


def test_swap_leaves_everything_else_alone():
    net = nn.Sequential(nn.Conv1d(6, 6, 3, groups=6), nn.Conv1d(6, 6, 3, groups=6, stride=2), nn.Conv1d(6, 6, 3, groups=6, padding=1),
                        nn.Conv1d(6, 6, 3, groups=3), nn.Conv1d(6, 12, 3, groups=6), nn.Conv1d(6, 6, 1),
                        nn.Conv1d(6, 6, 3, groups=6, padding_mode="replicate"), nn.Conv1d(6, 6, 33, groups=6),
                        nn.Conv1d(6, 6, 3, groups=6, dilation=128), nn.Conv2d(6, 6, (3, 1), groups=6),
                        depthwise.DepthwiseConv1d(6, 6, 3, groups=6), nn.Sequential(nn.Conv1d(4, 4, 5, dilation=2, groups=4, bias=False)))
    before = list(net)
    assert depthwise.use_device_depthwise_convs(net) == 2
    assert type(net[0]) is depthwise.DepthwiseConv1d and type(net[11][0]) is depthwise.DepthwiseConv1d and net[11][0].bias is None
    assert all(net[i] is before[i] for i in range(1, 11))
    assert net[0].weight is before[0].weight and net[0].bias is before[0].bias and net[0].training == before[0].training
    # on the CPU a swapped convolution is torch's own statement
    x = torch.randn(2, 6, 9)
    assert torch.equal(net[0](x), before[0](x))
    assert torch.equal(net[0](x, 2), before[0](F.pad(x, (2, 0))))
    assert torch.equal(net[1](x), before[1](x))
    # a DepthwiseConv1d that is no depthwise convolution (or is strided) is an nn.Conv1d with a left_pad
    dense = depthwise.DepthwiseConv1d(6, 4, 3, stride=2)
    assert torch.equal(dense(x, 1), F.conv1d(F.pad(x, (1, 0)), dense.weight, dense.bias, stride=2))


def test_limits_follow_the_plan():
    from tests import depthwise_conv_ref as dr
    for K, d in ((1, 1), (32, 8), (16, 17), (33, 1), (32, 9), (3, 128), (0, 1), (3, 0)):
        assert depthwise.in_device_limits(K, d) == dr.check(1, 1, max(1, (K - 1) * d + 1), K, d, 0), (K, d)
    assert not depthwise.in_device_limits("x", 1)


def test_depthwise_conv1d_refuses_cpu_tensors():
    with pytest.raises(ValueError, match="no CPU fallback"):
        depthwise.depthwise_conv1d(torch.zeros(1, 3, 9), torch.zeros(3, 1, 2))
