"""GPU: the one workspace a device that wekws_amd._device hands to the depthwise Conv1d, BatchNorm1d and the FSMN memory block.
Each layer's gradients computed alone are the reference; the three interleaved on the shared buffer, after the buffer has been
reallocated, and on a side stream must repeat them bit for bit (each kernel's bits are a function of its inputs and shape; the
kernels themselves are held to their oracles elsewhere).  The shapes are the smallest that still take the tile, fold and scalar
(T no multiple of 4) paths.  And require_float32's refusal of a device tensor by its dtype alone, which no CPU test can reach."""
import pytest
import torch

from wekws_amd import _device
from wekws_amd.model import batchnorm, depthwise, fsmn

pytestmark = pytest.mark.gpu


class _Layer:
    """A module, its inputs and an output gradient, all fixed; forward() and backward() are one differentiation of it."""

    def __init__(self, node, module, call, *shapes):
        self.node, self.module, self.call = node, module.cuda(), call
        self.inputs = [torch.randn(s).cuda() for s in shapes]
        self.g = None

    def forward(self):
        self.module.zero_grad(set_to_none=True)
        self.leaves = [t.clone().requires_grad_() for t in self.inputs]
        self.y = self.call(self.module, *self.leaves)
        assert type(self.y.grad_fn).__name__ == self.node          # the device call, not torch's own ops
        if self.g is None:
            self.g = torch.randn(self.y.shape).cuda()

    def backward(self):
        """The bits of every input and parameter gradient."""
        self.y.backward(self.g)
        grads = [t.grad for t in self.leaves] + [p.grad for p in self.module.parameters()]
        assert all(g is not None and g.dtype == torch.float32 for g in grads)
        return [g.view(torch.int32).cpu() for g in grads]


def _layers():
    torch.manual_seed(23)
    bn = batchnorm.DeviceBatchNorm1d(5).train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    return [_Layer("_DepthwiseConv1dBackward", depthwise.DepthwiseConv1d(5, 5, 3, dilation=2, groups=5), lambda m, x: m(x, left_pad=4),
                   (2, 5, 19)),
            _Layer("_BatchNormActBackward", bn, lambda m, x, r: m(x, residual=r, relu=True), (3, 5, 7), (3, 5, 7)),
            _Layer("_FsmnMemoryBackward", fsmn.FSMNBlock(6, 6, 3, 1, 1, 1), lambda m, x: m(x)[0], (2, 9, 6))]


def _interleaved(layers):
    for layer in layers:
        layer.forward()
    return [layer.backward() for layer in reversed(layers)][::-1]


def _same(got, want):
    return all(len(g) == len(w) and all(torch.equal(a, b) for a, b in zip(g, w)) for g, w in zip(got, want))


def test_three_layers_share_one_workspace_bit_for_bit():
    dev = torch.device("cuda", torch.cuda.current_device())
    _device._workspaces.pop(dev, None)                      # whatever ran before: start from no buffer
    layers = _layers()
    alone = []
    for layer in layers:
        layer.forward()
        alone.append(layer.backward())
    small = _device._workspaces[dev]                        # every layer took the device call, and its workspace from here
    assert [len(g) for g in alone] == [3, 4, 3] and all(bool(t.any()) for g in alone for t in g)

    assert _same(_interleaved(layers), alone)
    assert _device._workspaces[dev] is small

    big = torch.randn(4, 16, 64, device="cuda", requires_grad=True)
    batchnorm.DeviceBatchNorm1d(16).cuda().train()(big).sum().backward()
    grown = _device._workspaces[dev]
    assert grown is not small and grown.numel() > small.numel()
    assert _same(_interleaved(layers), alone)

    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        on_a_side_stream = _interleaved(layers)
    torch.cuda.synchronize()
    assert _same(on_a_side_stream, alone)
    assert _device._workspaces[dev] is grown


def test_require_float32_refuses_a_float64_device_tensor_by_its_dtype():
    x = torch.zeros(2, device="cuda")
    _device.require_float32("some_op", x, (("x", x), ("weight", x.clone())))
    with pytest.raises(ValueError) as err:
        _device.require_float32("some_op", x, (("x", x), ("weight", x.double())))
    assert str(err.value) == "some_op: weight must be a float32 tensor on a ROCm device (no CPU fallback)"
