"""The dense (``groups=1``) dilated Conv1d of the TCN backbone on the device: ``dense_conv1d`` is
``F.conv1d(F.pad(x, (left_pad, 0)), weight, bias, dilation=dilation)`` for a ``(Co, Ci, K)`` weight -- the reference's
``CnnBlock.cnn[0]`` behind its block's ``F.pad`` (wekws/model/tcn.py) and, with ``left_pad = 0``, ``Conv1dSubsampling1.out[0]``
(wekws/model/subsampling.py) -- and its autograd as HIP kernels with a stated arithmetic (csrc/dense_conv_plan.h,
csrc/dense_conv.hip.h): the forward product and the input gradient are float32 fmaf chains over the taps and, inside
a tap, the channels, ascending, on the exact-float32 matrix instruction, with the padding's zeros supplied by the kernel; the
weight gradient of every tap and the bias gradient are ``wekws_amd.model.linear``'s kernels -- float32 chains of 512 rows, added
and folded in double, rounded once -- fetching the tap's shifted ``(B, C, T)`` operand, all taps in one launch, so their bits are
those of ``linear_weight_grad`` on the shifted, zero-padded, transposed copies, which are never made.

``DenseConv1d`` is an ``nn.Conv1d``: the same constructor, parameters and state-dict keys, and a ``forward(input, left_pad=0)``.
``use_device_dense_convs(module)`` swaps every eligible ``nn.Conv1d`` below a module -- this package's and the reference's own --
for a ``DenseConv1d`` over the same Parameter objects.

The device path runs for contiguous 3-D float32 tensors on a ROCm device; everything else is ``nn.Conv1d.forward`` behind an
``F.pad``.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from wekws_amd import _capi, _device

MAX_CHANNELS = 65535        # csrc/dense_conv_plan.h: Ci and Co
MAX_TAPS = 32               # K
MAX_WINDOW = 256            # (K - 1) * dilation + 1


def in_device_limits(kernel_size, dilation) -> bool:
    """The limits of csrc/dense_conv_plan.h on a convolution's taps."""
    try:
        kernel_size, dilation = int(kernel_size), int(dilation)
    except (TypeError, ValueError):
        return False
    return 1 <= kernel_size <= MAX_TAPS and dilation >= 1 and (kernel_size - 1) * dilation + 1 <= MAX_WINDOW


class _DenseConv1d(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias, dilation, left_pad):
        B, Ci, Tin = x.shape
        Co, _, K = weight.shape
        x, w = x.contiguous(), weight.contiguous()
        b = bias.contiguous() if bias is not None else None
        y = torch.empty(B, Co, Tin + left_pad - (K - 1) * dilation, dtype=x.dtype, device=x.device)
        with _device.on(x.device):
            _capi.check(_capi.load().wekws_hip_dense_conv1d_forward(x.data_ptr(), B, Ci, Tin, w.data_ptr(), _device.ptr(b), Co, K, dilation,
                                                                    left_pad, y.data_ptr(), _device.stream(x.device)),
                        "wekws_hip_dense_conv1d_forward")
        ctx.save_for_backward(x, w)
        ctx.conf = (dilation, left_pad, bias is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, w = ctx.saved_tensors
        dilation, left_pad, has_bias = ctx.conf
        B, Ci, Tin = x.shape
        Co, _, K = w.shape
        want_x, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_b = has_bias and ctx.needs_input_grad[2]
        if not (want_x or want_w or want_b):
            return None, None, None, None, None
        g = grad_y.contiguous()
        dx = torch.empty_like(x) if want_x else None
        dw = torch.empty_like(w) if want_w else None
        db = torch.empty(Co, dtype=x.dtype, device=x.device) if want_b else None
        ws, ws_bytes = None, 0
        if want_w or want_b:
            ws_bytes = _device.library_bytes("wekws_hip_dense_conv1d_workspace_bytes", (B, Ci, Tin, Co, K, dilation, left_pad), ValueError,
                                             "dense_conv1d")
            ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=x.device)
        with _device.on(x.device):
            _capi.check(_capi.load().wekws_hip_dense_conv1d_backward(
                x.data_ptr(), g.data_ptr(), B, Ci, Tin, w.data_ptr(), Co, K, dilation, left_pad, _device.ptr(dx), _device.ptr(dw),
                _device.ptr(db), _device.ptr(ws), ws_bytes, _device.stream(x.device)), "wekws_hip_dense_conv1d_backward")
        return dx, dw, db, None, None


def dense_conv1d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, dilation: int = 1,
                 left_pad: int = 0) -> torch.Tensor:
    """``F.conv1d(F.pad(x, (left_pad, 0)), weight, bias, dilation=dilation)`` on the device, differentiable once: ``x``
    (B, Ci, Tin) float32 on a ROCm device, ``weight`` (Co, Ci, K) -- ``conv.weight`` as it is -- ``bias`` (Co) or None,
    ``0 <= left_pad <= (K - 1) * dilation``.  Returns y (B, Co, Tin + left_pad - (K - 1) * dilation).  The padding is not
    materialised.  Only the gradients autograd asks for are computed.  Non-contiguous inputs are made contiguous; the call runs
    on the current stream and reads nothing on the host.  No CPU fallback: anything else raises."""
    _device.require_float32("dense_conv1d", x, (("x", x), ("weight", weight)) + ((("bias", bias),) if bias is not None else ()))
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError(f"dense_conv1d: x must be (B, Ci, T) with no empty dimension, got {tuple(x.shape)}")
    Ci = x.shape[1]
    if weight.dim() != 3 or weight.shape[1] != Ci or min(weight.shape) < 1:
        raise ValueError(f"dense_conv1d: weight must be (Co, Ci, K) with Ci = {Ci}, got {tuple(weight.shape)}")
    Co, _, K = weight.shape
    if bias is not None and tuple(bias.shape) != (Co,):
        raise ValueError(f"dense_conv1d: bias must be ({Co},), got {tuple(bias.shape)}")
    if not (1 <= Ci <= MAX_CHANNELS and 1 <= Co <= MAX_CHANNELS):
        raise ValueError(f"dense_conv1d: 1 .. {MAX_CHANNELS} channels, got Ci={Ci} Co={Co}")
    dilation, left_pad = int(dilation), int(left_pad)
    if not in_device_limits(K, dilation):
        raise ValueError(f"dense_conv1d: K={K} dilation={dilation} outside the kernels' limits (1 <= K <= {MAX_TAPS}, dilation >= 1, "
                         f"a window of at most {MAX_WINDOW} frames)")
    if not 0 <= left_pad <= (K - 1) * dilation:
        raise ValueError(f"dense_conv1d: left_pad={left_pad} outside 0..(K-1)*dilation = {(K - 1) * dilation}")
    if x.shape[2] + left_pad - (K - 1) * dilation < 1:
        raise ValueError(f"dense_conv1d: {x.shape[2]} frames and left_pad={left_pad} are shorter than the window of "
                         f"{(K - 1) * dilation + 1} frames")
    return _DenseConv1d.apply(x, weight, bias, dilation, left_pad)


def _is_dense(conv: nn.Conv1d) -> bool:
    return (conv.groups == 1 and tuple(conv.stride) == (1,) and tuple(conv.padding) == (0,) and conv.padding_mode == "zeros"
            and conv.kernel_size[0] >= 2 and in_device_limits(conv.kernel_size[0], conv.dilation[0])
            and 1 <= conv.in_channels <= MAX_CHANNELS and 1 <= conv.out_channels <= MAX_CHANNELS)


class DenseConv1d(nn.Conv1d):
    """An ``nn.Conv1d`` -- the same constructor, parameters and state-dict keys -- whose ``forward(input, left_pad=0)`` is
    ``conv(F.pad(input, (left_pad, 0)))``: ``dense_conv1d`` for contiguous 3-D float32 device tensors when the convolution is
    dense (groups 1, stride 1, padding 0, zeros padding mode, ``kernel_size >= 2``), inside the kernels' limits and has an output
    frame, and ``nn.Conv1d.forward`` behind an ``F.pad`` otherwise, bit for bit.  The parameters may be views of an optimiser's
    flat buffers (``wekws_amd.optim.ClipAdam``)."""

    @classmethod
    def sharing(cls, conv: nn.Conv1d) -> "DenseConv1d":
        """A DenseConv1d over the very Parameter objects of ``conv``."""
        new = cls(conv.in_channels, conv.out_channels, conv.kernel_size[0], stride=conv.stride[0], padding=conv.padding[0],
                  dilation=conv.dilation[0], groups=conv.groups, bias=conv.bias is not None, padding_mode=conv.padding_mode,
                  device="meta")
        new.weight = conv.weight
        if conv.bias is not None:
            new.bias = conv.bias
        new.train(conv.training)
        return new

    def _on_device(self, x, left_pad) -> bool:
        w, b = self.weight, self.bias
        K, d = self.kernel_size[0], self.dilation[0]
        return (_is_dense(self) and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3
                and x.numel() > 0 and x.is_contiguous() and x.shape[1] == self.in_channels
                and w.is_cuda and w.dtype == torch.float32 and w.device == x.device
                and (b is None or (b.is_cuda and b.dtype == torch.float32 and b.device == x.device))
                and 0 <= left_pad <= (K - 1) * d and x.shape[2] + left_pad - (K - 1) * d >= 1)

    def forward(self, input, left_pad: int = 0):  # noqa: A002 (nn.Conv1d's own argument name)
        if self._on_device(input, left_pad):
            return dense_conv1d(input, self.weight, self.bias, self.dilation[0], left_pad)
        if left_pad:
            input = F.pad(input, (left_pad, 0), value=0.0)  # noqa: A001
        return super().forward(input)


def use_device_dense_convs(module: nn.Module) -> int:
    """Replace every child below ``module`` whose type is exactly ``nn.Conv1d`` and that is dense (groups 1, stride 1, padding 0,
    zeros padding mode, ``kernel_size >= 2``, inside the kernels' limits) by a ``DenseConv1d`` that shares its Parameter objects,
    so optimisers built before the swap, state dicts and the other ``use_device_*`` swaps stay valid in any order: a pointwise
    convolution (``kernel_size == 1``) is ``use_device_pointwise_convs``'s and a depthwise one (``groups == channels``, more than
    one channel) ``use_device_depthwise_convs``'s, never this swap's.  Idempotent: what is swapped already is left alone.  Returns
    the number swapped."""
    return _device.swap_children(module, lambda child: type(child) is nn.Conv1d and _is_dense(child), DenseConv1d.sharing)
