"""The pointwise (``kernel_size=1``) Conv1d of the TCN and MDTC backbones on the device: ``pointwise_conv1d`` is
``F.conv1d(x, weight, bias)`` for a ``(Co, Ci, 1)`` weight -- the reference's ``DsCnnBlock.cnn[3]`` (wekws/model/tcn.py),
``DSDilatedConv1d.pointwise`` and ``TCNBlock.conv2`` (wekws/model/mdtc.py) -- and its autograd as HIP kernels with a stated
arithmetic (csrc/pointwise_conv_plan.h, csrc/pointwise_conv.hip.h): the forward product and the input gradient
are float32 fmaf chains over the channels, ascending, on the exact-float32 matrix instruction; the weight and bias gradients are
``wekws_amd.model.linear``'s kernels -- float32 chains of 512 rows, added and folded in double, rounded once -- fetching
``(B, C, T)`` operands, so their bits are those of ``linear_weight_grad`` on the transposed copies, which are never made.

``PointwiseConv1d`` is an ``nn.Conv1d``: the same constructor, parameters and state-dict keys.
``use_device_pointwise_convs(module)`` swaps every eligible ``nn.Conv1d`` below a module -- this package's and the reference's
own -- for a ``PointwiseConv1d`` over the same Parameter objects.

The device path runs for contiguous 3-D float32 tensors on a ROCm device with at least one frame; everything else is
``nn.Conv1d.forward``.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from wekws_amd import _capi, _device

MAX_CHANNELS = 65535        # csrc/pointwise_conv_plan.h: Ci and Co


class _PointwiseConv1d(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias):
        B, Ci, T = x.shape
        Co = weight.shape[0]
        x, w = x.contiguous(), weight.contiguous()
        b = bias.contiguous() if bias is not None else None
        y = torch.empty(B, Co, T, dtype=x.dtype, device=x.device)
        with _device.on(x.device):
            _capi.check(_capi.load().wekws_hip_pointwise_conv1d_forward(x.data_ptr(), B, Ci, T, w.data_ptr(), _device.ptr(b), Co,
                                                                        y.data_ptr(), _device.stream(x.device)),
                        "wekws_hip_pointwise_conv1d_forward")
        ctx.save_for_backward(x, w)
        ctx.conf = (weight.shape, bias is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, w = ctx.saved_tensors
        w_shape, has_bias = ctx.conf
        B, Ci, T = x.shape
        Co = w.shape[0]
        want_x, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_b = has_bias and ctx.needs_input_grad[2]
        if not (want_x or want_w or want_b):
            return None, None, None
        g = grad_y.contiguous()
        dx = torch.empty_like(x) if want_x else None
        dw = torch.empty(Co, Ci, dtype=x.dtype, device=x.device) if want_w else None
        db = torch.empty(Co, dtype=x.dtype, device=x.device) if want_b else None
        ws, ws_bytes = None, 0
        if want_w or want_b:
            ws_bytes = _device.library_bytes("wekws_hip_pointwise_conv1d_workspace_bytes", (B, Ci, T, Co), ValueError, "pointwise_conv1d")
            ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=x.device)
        with _device.on(x.device):
            _capi.check(_capi.load().wekws_hip_pointwise_conv1d_backward(
                x.data_ptr(), g.data_ptr(), B, Ci, T, w.data_ptr(), Co, _device.ptr(dx), _device.ptr(dw), _device.ptr(db), _device.ptr(ws),
                ws_bytes, _device.stream(x.device)), "wekws_hip_pointwise_conv1d_backward")
        return dx, dw.view(w_shape) if want_w else None, db


def pointwise_conv1d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.conv1d(x, weight, bias)`` for a pointwise weight, on the device, differentiable once: ``x`` (B, Ci, T) float32 on a
    ROCm device, ``weight`` (Co, Ci, 1) -- ``conv.weight`` as it is -- or (Co, Ci), ``bias`` (Co) or None.  Returns y (B, Co, T).
    Only the gradients autograd asks for are computed.  Non-contiguous inputs are made contiguous; the call runs on the current
    stream and reads nothing on the host.  No CPU fallback: anything else raises."""
    _device.require_float32("pointwise_conv1d", x, (("x", x), ("weight", weight)) + ((("bias", bias),) if bias is not None else ()))
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError(f"pointwise_conv1d: x must be (B, Ci, T) with no empty dimension, got {tuple(x.shape)}")
    Ci = x.shape[1]
    if weight.dim() not in (2, 3) or weight.shape[1] != Ci or weight.shape[0] < 1 or (weight.dim() == 3 and weight.shape[2] != 1):
        raise ValueError(f"pointwise_conv1d: weight must be (Co, Ci, 1) or (Co, Ci) with Ci = {Ci}, got {tuple(weight.shape)}")
    Co = weight.shape[0]
    if bias is not None and tuple(bias.shape) != (Co,):
        raise ValueError(f"pointwise_conv1d: bias must be ({Co},), got {tuple(bias.shape)}")
    if not (1 <= Ci <= MAX_CHANNELS and 1 <= Co <= MAX_CHANNELS):
        raise ValueError(f"pointwise_conv1d: 1 .. {MAX_CHANNELS} channels, got Ci={Ci} Co={Co}")
    return _PointwiseConv1d.apply(x, weight, bias)


def _is_pointwise(conv: nn.Conv1d) -> bool:
    return (tuple(conv.kernel_size) == (1,) and tuple(conv.stride) == (1,) and tuple(conv.padding) == (0,)
            and tuple(conv.dilation) == (1,) and conv.groups == 1 and conv.padding_mode == "zeros"
            and 1 <= conv.in_channels <= MAX_CHANNELS and 1 <= conv.out_channels <= MAX_CHANNELS)


class PointwiseConv1d(nn.Conv1d):
    """An ``nn.Conv1d`` -- the same constructor, parameters and state-dict keys -- whose ``forward`` is ``pointwise_conv1d`` for
    contiguous 3-D float32 device tensors when the convolution is pointwise (``kernel_size == (1,)``, stride 1, padding 0,
    dilation 1, groups 1, zeros padding mode), and ``nn.Conv1d.forward`` otherwise, bit for bit.  The parameters may be views of
    an optimiser's flat buffers (``wekws_amd.optim.ClipAdam``)."""

    @classmethod
    def sharing(cls, conv: nn.Conv1d) -> "PointwiseConv1d":
        """A PointwiseConv1d over the very Parameter objects of ``conv``."""
        new = cls(conv.in_channels, conv.out_channels, conv.kernel_size[0], stride=conv.stride[0], padding=conv.padding[0],
                  dilation=conv.dilation[0], groups=conv.groups, bias=conv.bias is not None, padding_mode=conv.padding_mode,
                  device="meta")
        new.weight = conv.weight
        if conv.bias is not None:
            new.bias = conv.bias
        new.train(conv.training)
        return new

    def _on_device(self, x) -> bool:
        w, b = self.weight, self.bias
        return (_is_pointwise(self) and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3
                and x.numel() > 0 and x.is_contiguous() and x.shape[1] == self.in_channels
                and w.is_cuda and w.dtype == torch.float32 and w.device == x.device
                and (b is None or (b.is_cuda and b.dtype == torch.float32 and b.device == x.device)))

    def forward(self, input):  # noqa: A002 (nn.Conv1d's own argument name)
        if not self._on_device(input):
            return super().forward(input)
        return pointwise_conv1d(input, self.weight, self.bias)


def use_device_pointwise_convs(module: nn.Module) -> int:
    """Replace every child below ``module`` whose type is exactly ``nn.Conv1d`` and that is pointwise (``kernel_size == (1,)``,
    stride 1, padding 0, dilation 1, groups 1, zeros padding mode) by a ``PointwiseConv1d`` that shares its Parameter objects, so
    optimisers built before the swap, state dicts and the other ``use_device_*`` swaps stay valid in any order.  Idempotent: what
    is swapped already is left alone.  Returns the number swapped."""
    return _device.swap_children(module, lambda child: type(child) is nn.Conv1d and _is_pointwise(child), PointwiseConv1d.sharing)
