"""The depthwise Conv1d of the TCN and MDTC backbones on the device: ``depthwise_conv1d`` is
``F.conv1d(F.pad(x, (left_pad, 0)), weight, bias, dilation=dilation, groups=C)`` -- the reference's ``DsCnnBlock.cnn[0]``
(wekws/model/tcn.py:102-107) and ``DSDilatedConv1d.conv`` (wekws/model/mdtc.py:37-46) behind their blocks' ``F.pad`` -- and its
autograd as three HIP kernels (csrc/depthwise_conv.hip.h): a causal FIR per (batch, channel) row that supplies
the padding's zeros itself, its mirror image for the input gradient, and a fixed-order double sum for the tap and bias gradients.

``DepthwiseConv1d`` is an ``nn.Conv1d`` with the same constructor, parameters and state-dict keys whose ``forward`` takes the
device call where it can; ``use_device_depthwise_convs(module)`` swaps the depthwise convolutions of any module -- the
reference's own ``TCN`` or ``MDTC`` included -- for ``DepthwiseConv1d``s that share their parameter objects.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from wekws_amd import _capi, _device

MAX_TAPS = 32          # K                                        (csrc/depthwise_conv_plan.h)
MAX_WINDOW = 256       # (K - 1) * dilation + 1


def in_device_limits(kernel_size, dilation) -> bool:
    """The limits of csrc/depthwise_conv_plan.h on a convolution's parameters."""
    try:
        kernel_size, dilation = int(kernel_size), int(dilation)
    except (TypeError, ValueError):
        return False
    return 1 <= kernel_size <= MAX_TAPS and dilation >= 1 and (kernel_size - 1) * dilation + 1 <= MAX_WINDOW


class _DepthwiseConv1d(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias, dilation, left_pad):
        B, C, Tin = x.shape
        K = weight.numel() // C
        x, w = x.contiguous(), weight.contiguous()
        b = bias.contiguous() if bias is not None else None
        y = torch.empty(B, C, Tin + left_pad - (K - 1) * dilation, dtype=x.dtype, device=x.device)
        with _device.on(x.device):
            _capi.check(_capi.load().wekws_hip_depthwise_conv1d_forward(x.data_ptr(), B, C, Tin, w.data_ptr(), _device.ptr(b), K, dilation,
                                                                        left_pad, y.data_ptr(), _device.stream(x.device)),
                        "wekws_hip_depthwise_conv1d_forward")
        ctx.save_for_backward(x, w)
        ctx.conf = (dilation, left_pad, weight.shape, bias is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, w = ctx.saved_tensors
        dilation, left_pad, w_shape, has_bias = ctx.conf
        B, C, Tin = x.shape
        K = w.numel() // C
        want_x, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_b = has_bias and ctx.needs_input_grad[2]
        if not (want_x or want_w or want_b):
            return None, None, None, None, None
        g = grad_y.contiguous()
        lib = _capi.load()
        dx = torch.empty_like(x) if want_x else None
        dw = torch.empty_like(w) if want_w else None
        db = torch.empty(C, dtype=x.dtype, device=x.device) if want_b else None
        ws, ws_bytes = None, 0
        if want_w or want_b:
            ws_bytes = _device.library_bytes("wekws_hip_depthwise_conv1d_workspace_bytes", (B, C, Tin, K, dilation, left_pad),
                                             _capi.HipLibraryError)
            ws = _device.workspace(x.device, ws_bytes)
        with _device.on(x.device):
            _capi.check(lib.wekws_hip_depthwise_conv1d_backward(
                x.data_ptr(), g.data_ptr(), B, C, Tin, w.data_ptr(), K, dilation, left_pad, _device.ptr(dx), _device.ptr(dw),
                _device.ptr(db), _device.ptr(ws), ws_bytes, _device.stream(x.device)), "wekws_hip_depthwise_conv1d_backward")
        return dx, dw.view(w_shape) if want_w else None, db, None, None


def depthwise_conv1d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, dilation: int = 1,
                     left_pad: int = 0) -> torch.Tensor:
    """``F.conv1d(F.pad(x, (left_pad, 0)), weight, bias, dilation=dilation, groups=C)`` on the device, differentiable once:
    ``x`` (B, C, Tin) float32 on a ROCm device, ``weight`` (C, 1, K) -- ``conv.weight`` as it is -- or (C, K), ``bias`` (C) or
    None, ``0 <= left_pad <= (K - 1) * dilation``.  Returns y (B, C, Tin + left_pad - (K - 1) * dilation).  The padding is not
    materialised.  Non-contiguous inputs are made contiguous; the call runs on the current stream and reads nothing on the
    host.  No CPU fallback: anything else raises."""
    _device.require_float32("depthwise_conv1d", x, (("x", x), ("weight", weight)) + ((("bias", bias),) if bias is not None else ()))
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError(f"depthwise_conv1d: x must be (B, C, T) with no empty dimension, got {tuple(x.shape)}")
    C = x.shape[1]
    if weight.dim() not in (2, 3) or weight.shape[0] != C or weight.numel() == 0 or (weight.dim() == 3 and weight.shape[1] != 1):
        raise ValueError(f"depthwise_conv1d: weight must be (C, 1, K) or (C, K) with C = {C}, got {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (C,):
        raise ValueError(f"depthwise_conv1d: bias must be ({C},), got {tuple(bias.shape)}")
    K, dilation, left_pad = weight.numel() // C, int(dilation), int(left_pad)
    if not in_device_limits(K, dilation):
        raise ValueError(f"depthwise_conv1d: K={K} dilation={dilation} outside the kernels' limits (1 <= K <= {MAX_TAPS}, "
                         f"dilation >= 1, a window of at most {MAX_WINDOW} frames)")
    if not 0 <= left_pad <= (K - 1) * dilation:
        raise ValueError(f"depthwise_conv1d: left_pad={left_pad} outside 0..(K-1)*dilation = {(K - 1) * dilation}")
    if x.shape[2] + left_pad - (K - 1) * dilation < 1:
        raise ValueError(f"depthwise_conv1d: {x.shape[2]} frames and left_pad={left_pad} are shorter than the window of "
                         f"{(K - 1) * dilation + 1} frames")
    return _DepthwiseConv1d.apply(x, weight, bias, dilation, left_pad)


def _is_depthwise(conv: nn.Conv1d) -> bool:
    return (conv.groups == conv.in_channels == conv.out_channels and tuple(conv.stride) == (1,) and tuple(conv.padding) == (0,)
            and conv.padding_mode == "zeros" and in_device_limits(conv.kernel_size[0], conv.dilation[0]))


class DepthwiseConv1d(nn.Conv1d):
    """An ``nn.Conv1d`` -- the same constructor, parameters and state-dict keys -- whose ``forward(x, left_pad=0)`` is
    ``conv(F.pad(x, (left_pad, 0)))``: by the device call for float32 device tensors when the convolution is depthwise
    (``groups == in_channels == out_channels``, stride 1, no padding of its own) and inside the kernels' limits, by torch's own
    statement otherwise."""

    @classmethod
    def sharing(cls, conv: nn.Conv1d) -> "DepthwiseConv1d":
        """A DepthwiseConv1d over the very parameter objects of ``conv``."""
        new = cls(conv.in_channels, conv.out_channels, conv.kernel_size[0], stride=conv.stride[0], padding=conv.padding[0],
                  dilation=conv.dilation[0], groups=conv.groups, bias=conv.bias is not None, padding_mode=conv.padding_mode)
        new.weight = conv.weight
        new.bias = conv.bias
        new.train(conv.training)
        return new

    def _on_device(self, x: torch.Tensor, left_pad: int) -> bool:
        K, d = self.kernel_size[0], self.dilation[0]
        return (_is_depthwise(self) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.numel() > 0
                and x.shape[1] == self.in_channels and self.weight.is_cuda and self.weight.dtype == torch.float32
                and (self.bias is None or self.bias.dtype == torch.float32)
                and 0 <= left_pad <= (K - 1) * d and x.shape[2] + left_pad - (K - 1) * d >= 1)

    def forward(self, x: torch.Tensor, left_pad: int = 0) -> torch.Tensor:
        if self._on_device(x, left_pad):
            return depthwise_conv1d(x, self.weight, self.bias, self.dilation[0], left_pad)
        if left_pad:
            x = F.pad(x, (left_pad, 0), value=0.0)
        return super().forward(x)


def use_device_depthwise_convs(module: nn.Module) -> int:
    """Replace every ``nn.Conv1d`` below ``module`` that is depthwise (``groups == in_channels == out_channels``), has stride 1,
    no padding of its own, ``padding_mode == "zeros"`` and lies inside the kernels' limits by a ``DepthwiseConv1d`` that shares
    its parameter objects, so optimisers built before the swap and state dicts stay valid.  Everything else is left alone, and
    so are convolutions that are ``DepthwiseConv1d``s already.  Returns the number swapped."""
    return _device.swap_children(
        module, lambda child: not isinstance(child, DepthwiseConv1d) and isinstance(child, nn.Conv1d) and _is_depthwise(child),
        DepthwiseConv1d.sharing)
