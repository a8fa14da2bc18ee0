"""CPU: wekws_amd.model.batchnorm without a device -- the BatchNorm swap (counts, shared parameter and buffer objects, state-dict
keys, idempotence), ``DeviceBatchNorm1d`` as torch's own statements on CPU tensors, and the mirrors of wekws_amd.model.tcn / .mdtc
with ``fused_norm`` set against the unfused ones bit for bit."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from wekws_amd.model import batchnorm, mdtc, tcn

MODELS = {
    "tcn_ds": (lambda: tcn.TCN(4, 64, 8, block_class=tcn.DsCnnBlock), 64, 8),
    "mdtc_small": (lambda: mdtc.MDTC(3, 4, 32, 32, 5, True), 32, 39),
    "tcn_tiny_cnn": (lambda: tcn.TCN(2, 8, 3, block_class=tcn.CnnBlock), 8, 2),
    "mdtc_tiny_sq": (lambda: mdtc.MDTC(2, 2, 8, 8, 3, True), 8, 15),
}


@pytest.mark.parametrize("tag", sorted(MODELS))
def test_swap_counts_shares_and_is_idempotent(tag):
    make, _, count = MODELS[tag]
    model = make()
    params, buffers, keys = list(model.parameters()), list(model.buffers()), list(model.state_dict())
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    assert sum(isinstance(m, nn.BatchNorm1d) for m in model.modules()) == count
    assert not any(getattr(m, "fused_norm", False) for m in model.modules())
    assert batchnorm.use_device_batchnorms(model) == count
    assert sum(isinstance(m, batchnorm.DeviceBatchNorm1d) for m in model.modules()) == count
    assert sum(type(m) is nn.BatchNorm1d for m in model.modules()) == 0
    after_p, after_b = list(model.parameters()), list(model.buffers())
    assert len(after_p) == len(params) and all(a is b for a, b in zip(after_p, params))      # the very objects an optimiser holds
    assert len(after_b) == len(buffers) and all(a is b for a, b in zip(after_b, buffers))
    assert all(p is q for p, q in zip(opt.param_groups[0]["params"], after_p))
    assert list(model.state_dict()) == keys
    ours = [m for m in model.modules() if isinstance(m, (tcn.DsCnnBlock, mdtc.DSDilatedConv1d, mdtc.TCNBlock))]
    assert all(m.fused_norm is True for m in ours) and (ours or tag == "tcn_tiny_cnn")
    assert not any(getattr(m, "fused_norm", False) for m in model.modules() if isinstance(m, tcn.CnnBlock))
    assert batchnorm.use_device_batchnorms(model) == 0
    assert list(model.state_dict()) == keys and all(a is b for a, b in zip(model.buffers(), buffers))
    # a state dict saved before the swap loads after it, and the other way round
    fresh = make()
    fresh.load_state_dict(model.state_dict())
    model.load_state_dict(fresh.state_dict())


def test_fused_norm_defaults_to_the_unfused_statements():
    assert tcn.DsCnnBlock.fused_norm is False and mdtc.DSDilatedConv1d.fused_norm is False and mdtc.TCNBlock.fused_norm is False
    assert not hasattr(tcn.CnnBlock, "fused_norm")


def test_swap_serves_every_kind_of_batchnorm_and_leaves_the_rest():
    net = nn.Sequential(nn.BatchNorm1d(6), nn.BatchNorm1d(6, affine=False), nn.BatchNorm1d(6, track_running_stats=False),
                        nn.BatchNorm1d(6, momentum=None, eps=1e-3), nn.BatchNorm2d(6), nn.LayerNorm(6), batchnorm.DeviceBatchNorm1d(6),
                        nn.Sequential(nn.BatchNorm1d(4).eval()))
    before = list(net)
    assert batchnorm.use_device_batchnorms(net) == 5
    assert all(type(net[i]) is batchnorm.DeviceBatchNorm1d for i in range(4)) and type(net[7][0]) is batchnorm.DeviceBatchNorm1d
    assert all(net[i] is before[i] for i in (4, 5, 6))
    assert net[1].weight is None and net[1].bias is None and net[1].running_mean is before[1].running_mean
    assert net[2].running_mean is None and net[2].num_batches_tracked is None and net[2].weight is before[2].weight
    assert net[3].momentum is None and net[3].eps == 1e-3 and net[3].num_batches_tracked is before[3].num_batches_tracked
    assert net[0].training and not net[7][0].training
    # on the CPU a swapped BatchNorm is torch's own statements, buffers included
    x, res = torch.randn(3, 6, 5), torch.randn(3, 6, 5)
    for i in range(4):
        twin = copy.deepcopy(before[i])
        for mode in (True, False):
            net[i].train(mode)
            twin.train(mode)
            assert torch.equal(net[i](x), twin(x))
            assert torch.equal(net[i](x, relu=True), F.relu(twin(x)))
            assert torch.equal(net[i](x, residual=res, relu=True), F.relu(twin(x) + res))
            assert torch.equal(net[i](x, residual=res), twin(x) + res)
            assert torch.equal(net[i](x[:, :, 0]), twin(x[:, :, 0]))
        for a, b in zip(net[i].buffers(), twin.buffers()):
            assert torch.equal(a, b)


def _run(model, x, mode):
    model.train(mode)
    torch.manual_seed(3)                                   # (dropout draws the same mask in both models)
    y, cache = model(x)
    y1, cache1 = model(x[:, :5])
    y2, cache2 = model(x[:, 5:], cache1)
    return [y, cache, y1, cache1, y2, cache2]


@pytest.mark.parametrize("tag", sorted(MODELS))
def test_fused_mirrors_equal_the_unfused_ones_bit_for_bit(tag):
    """train() and eval(), one shot and in two chunks with a carried cache, outputs, gradients and buffers."""
    make, D, _ = MODELS[tag]
    torch.manual_seed(1)
    plain = make()
    fused = copy.deepcopy(plain)
    batchnorm.use_device_batchnorms(fused)
    x = torch.randn(3, 11, D)
    for mode in (True, False, True):
        a, b = _run(plain, x, mode), _run(fused, x, mode)
        assert all(torch.equal(u, v) for u, v in zip(a, b)), (tag, mode)
        for (n, u), v in zip(plain.state_dict().items(), fused.state_dict().values()):
            assert torch.equal(u, v), (tag, mode, n)
    for m in (plain, fused):
        m.train()
        torch.manual_seed(4)
        m(x)[0].square().sum().backward()
    for (n, p), q in zip(plain.named_parameters(), fused.parameters()):
        assert torch.equal(p.grad, q.grad), n


def test_batch_norm_act_refuses_cpu_tensors():
    with pytest.raises(ValueError, match="no CPU fallback"):
        batchnorm.batch_norm_act(torch.zeros(2, 3, 9), None, None, None, None, None, True, 0.1, 1e-5)
