"""CPU: what of wekws_amd.model.linear runs without a device -- DeviceLinear and use_device_weight_grads on CPU tensors are torch
bit for bit, Parameter objects and state-dict keys are shared, the swap counts for the recipe's FSMN and for a GRU keyword
model, idempotence, and the ``device_weight_grads`` switch of DeviceGRU, off by default."""
import copy
import inspect

import pytest
import torch
import torch.nn as nn

from wekws_amd.model import fsmn
from wekws_amd.model import gru as dg
from wekws_amd.model import linear as dl


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", [(7, 20), (3, 5, 20), (20,), (0, 20)])
def test_device_linear_on_cpu_tensors_is_nn_linear(bias, shape):
    torch.manual_seed(3)
    ref = nn.Linear(20, 24, bias=bias)
    dev = dl.DeviceLinear(20, 24, bias=bias)
    assert list(dev.state_dict()) == list(ref.state_dict())
    dev.load_state_dict(ref.state_dict())
    x = torch.randn(*shape)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya, yb = ref(xa), dev(xb)
    ya.sum().backward()
    yb.sum().backward()
    assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    for a, b in zip(ref.parameters(), dev.parameters()):
        assert torch.equal(a.grad, b.grad)


def test_sharing_keeps_the_parameter_objects_and_the_mode():
    ref = nn.Linear(5, 3).eval()
    dev = dl.DeviceLinear.sharing(ref)
    assert dev.weight is ref.weight and dev.bias is ref.bias and not dev.training
    assert (dev.in_features, dev.out_features) == (5, 3) and list(dev.state_dict()) == ["weight", "bias"]
    nob = dl.DeviceLinear.sharing(nn.Linear(5, 3, bias=False))
    assert nob.bias is None and list(nob.state_dict()) == ["weight"]
    ref2 = nn.Linear(5, 3)
    ref2.load_state_dict(dev.state_dict())                                          # state dicts go both ways
    assert torch.equal(ref2.weight, ref.weight)


class _GruKws(nn.Module):
    """The reference's KWSModel for the gru recipe, as far as its modules go."""

    def __init__(self):
        super().__init__()
        self.preprocessing = nn.Sequential(nn.Linear(20, 16), nn.ReLU())
        self.backbone = nn.GRU(16, 16, num_layers=2, batch_first=True)
        self.classifier = nn.Linear(16, 2)

    def forward(self, x):
        y, _ = self.backbone(self.preprocessing(x))
        return torch.sigmoid(self.classifier(y))


def test_swap_counts_shared_parameters_and_idempotence():
    torch.manual_seed(5)
    net = fsmn.FSMN(400, 140, 4, 250, 128, 10, 2, 1, 1, 140, 2599)                   # examples/hi_xiaowen/s0/conf/fsmn_ctc.yaml
    twin = copy.deepcopy(net)
    before, keys = dict(net.named_parameters()), list(net.state_dict())
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    assert dl.use_device_weight_grads(net) == 12                                     # 4 affines and 2 Linears in each of 4 units
    assert sum(type(m) is dl.DeviceLinear for m in net.modules()) == 12 and not any(type(m) is nn.Linear for m in net.modules())
    after = dict(net.named_parameters())
    assert list(after) == list(before) and all(after[n] is before[n] for n in before) and list(net.state_dict()) == keys
    assert dl.use_device_weight_grads(net) == 0                                      # idempotent
    # on the CPU the swapped model is torch bit for bit, and the optimiser built before the swap still steps it
    x = torch.randn(2, 6, 400)
    ya, _ = net(x)
    yb, _ = twin(x)
    ya.sum().backward()
    yb.sum().backward()
    assert torch.equal(ya, yb)
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(net.parameters(), twin.parameters()))
    opt.step()
    assert not torch.equal(net.out_linear2.linear.weight, twin.out_linear2.linear.weight)


def test_gru_keyword_model_counts_and_the_switch():
    torch.manual_seed(6)
    net = _GruKws()
    twin = copy.deepcopy(net)
    assert dl.use_device_weight_grads(net) == 2 and type(net.backbone) is nn.GRU     # a torch GRU is not the swap's business
    assert dg.use_device_grus(net) == 1 and net.backbone.device_weight_grads is False
    assert dl.use_device_weight_grads(net) == 1 and net.backbone.device_weight_grads is True
    assert dl.use_device_weight_grads(net) == 0
    fresh = _GruKws()
    assert dg.use_device_grus(fresh) == 1 and dl.use_device_weight_grads(fresh) == 3
    assert dg.DeviceGRU.sharing(fresh.backbone).device_weight_grads is True and copy.deepcopy(fresh).backbone.device_weight_grads is True
    x = torch.randn(3, 5, 20)
    net.load_state_dict(twin.state_dict())
    ya, yb = net(x), twin(x)
    ya.sum().backward()
    yb.sum().backward()
    assert torch.equal(ya, yb) and all(torch.equal(a.grad, b.grad) for a, b in zip(net.parameters(), twin.parameters()))


def test_the_switch_defaults_to_off():
    assert dg.DeviceGRU(8, 16, batch_first=True).device_weight_grads is False
    assert dg.DeviceGRU(8, 16, batch_first=True, device_weight_grads=True).device_weight_grads is True
    assert dg.DeviceGRU.sharing(nn.GRU(8, 16, batch_first=True)).device_weight_grads is False
    assert inspect.signature(dg.gru_scan).parameters["device_weight_grads"].default is False
    assert list(dg.DeviceGRU(8, 16, device_weight_grads=True).state_dict()) == list(nn.GRU(8, 16).state_dict())


def test_subclasses_of_linear_keep_their_forward():
    class Odd(nn.Linear):
        def forward(self, x):
            return super().forward(x) * 2

    net = nn.Sequential(Odd(4, 4), nn.Linear(4, 4))
    assert dl.use_device_weight_grads(net) == 1 and type(net[0]) is Odd and type(net[1]) is dl.DeviceLinear
