"""BatchNorm1d of the TCN and MDTC backbones on the device, with the ReLU and the residual add that follow it fused in:
``batch_norm_act`` is ``relu(F.batch_norm(x, ...) + residual)`` -- the reference's ``DsCnnBlock.cnn[1:3]`` / ``[4:6]``
(wekws/model/tcn.py), ``DSDilatedConv1d.bn``, ``TCNBlock.bn1`` / ``relu1`` and ``TCNBlock.bn2`` + ``inputs`` + ``relu2``
(wekws/model/mdtc.py) -- and its autograd as one node over six HIP kernels (csrc/batchnorm.hip.h): double sums
in a fixed order for the statistics and the parameter gradients, one elementwise pass for ``y`` and one for ``grad_x``.  The
running buffers and ``num_batches_tracked`` are updated on the device; nothing is read on the host.

``DeviceBatchNorm1d`` is an ``nn.BatchNorm1d`` with the same constructor, parameters, buffers and state-dict keys whose
``forward(x, residual=None, relu=False)`` takes the device call where it can; ``use_device_batchnorms(module)`` swaps the
``nn.BatchNorm1d``s of any module for ``DeviceBatchNorm1d``s that share their parameter and buffer objects and switches this
package's own blocks to the fused calls.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from wekws_amd import _capi, _device


def _workspace_for(device: torch.device, B: int, C: int, T: int) -> torch.Tensor:
    """The workspace for a shape."""
    return _device.workspace(device, _device.library_bytes("wekws_hip_batchnorm_workspace_bytes", (B, C, T), ValueError))


def _check(rc: int, what: str) -> None:
    """The C checks' refusals are the caller's mistakes: ValueError; anything else is the library's error."""
    if rc == -1:
        raise ValueError(f"{what}: {_capi.last_error()}")
    _capi.check(rc, what)


class _BatchNormAct(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, num_batches_tracked, batch_stats, momentum, eps, relu):
        shape = x.shape
        B, C = shape[0], shape[1]
        T = shape[2] if x.dim() == 3 else 1
        x = x.contiguous()
        w = weight.contiguous() if weight is not None else None
        b = bias.contiguous() if bias is not None else None
        r = residual.contiguous() if residual is not None else None
        lib = _capi.load()
        y = torch.empty_like(x)
        stats = torch.empty(2, C, dtype=x.dtype, device=x.device)          # save_mean, save_invstd
        ws = _workspace_for(x.device, B, C, T)
        update = batch_stats and running_mean is not None
        ptr = _device.ptr
        with _device.on(x.device):
            _check(lib.wekws_hip_batchnorm_forward(
                x.data_ptr(), ptr(r), B, C, T, ptr(w), ptr(b), ptr(running_mean) if update or not batch_stats else None,
                ptr(running_var) if update or not batch_stats else None, ptr(num_batches_tracked) if update else None,
                int(batch_stats), -1.0 if momentum is None else float(momentum), float(eps), int(relu), y.data_ptr(), stats.data_ptr(),
                stats.data_ptr() + 4 * C, ws.data_ptr(), ws.numel(), _device.stream(x.device)), "wekws_hip_batchnorm_forward")
        ctx.save_for_backward(x, w, stats, y if relu else None)
        ctx.conf = (B, C, T, bool(batch_stats), bool(relu), weight is not None, bias is not None, residual is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, w, stats, y = ctx.saved_tensors
        B, C, T, batch_stats, relu, has_w, has_b, has_r = ctx.conf
        want_x = ctx.needs_input_grad[0]
        want_w = has_w and ctx.needs_input_grad[1]
        want_b = has_b and ctx.needs_input_grad[2]
        want_r = has_r and ctx.needs_input_grad[3]
        none = (None,) * 7
        g = grad_y.contiguous()
        if want_r and not relu:
            dres, want_r = g, False                                # grad_residual is grad_y itself: no pass
        else:
            dres = torch.empty_like(x) if want_r else None
        if not (want_x or want_w or want_b or want_r):
            return (None, None, None, dres) + none
        lib = _capi.load()
        dx = torch.empty_like(x) if want_x else None
        dw = torch.empty(C, dtype=x.dtype, device=x.device) if want_w else None
        db = torch.empty(C, dtype=x.dtype, device=x.device) if want_b else None
        ws = _workspace_for(x.device, B, C, T)
        ptr = _device.ptr
        with _device.on(x.device):
            _check(lib.wekws_hip_batchnorm_backward(
                x.data_ptr(), ptr(y), g.data_ptr(), B, C, T, ptr(w), stats.data_ptr(), stats.data_ptr() + 4 * C, int(batch_stats), int(relu),
                ptr(dx), ptr(dres) if want_r else None, ptr(dw), ptr(db), ws.data_ptr(), ws.numel(), _device.stream(x.device)),
                "wekws_hip_batchnorm_backward")
        return (dx, dw, db, dres) + none


def batch_norm_act(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], running_mean: Optional[torch.Tensor],
                   running_var: Optional[torch.Tensor], num_batches_tracked: Optional[torch.Tensor], training: bool,
                   momentum: Optional[float], eps: float, relu: bool = False, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.batch_norm(x, running_mean, running_var, weight, bias, training, momentum, eps)``, then ``+ residual`` when there is
    one, then ``relu`` when asked, on the device and differentiable once: ``x`` and ``residual`` (B, C, T) or (B, C) float32 on
    a ROCm device, the rest (C) float32 or None, ``num_batches_tracked`` an int64 scalar tensor or None.  ``training`` selects
    the batch statistics and the update of the running buffers, as in ``F.batch_norm``; without running buffers the batch
    statistics are used either way.  ``momentum=None`` is the cumulative average over ``num_batches_tracked``, which is
    incremented on the device together with the buffers.  Runs on the current stream and reads nothing on the host.  No CPU
    fallback: anything else raises ``ValueError``."""
    tensors = (("x", x), ("weight", weight), ("bias", bias), ("running_mean", running_mean), ("running_var", running_var),
               ("residual", residual))
    _device.require_float32("batch_norm_act", x, [(name, t) for name, t in tensors if t is not None or name == "x"])
    if x.dim() not in (2, 3) or min(x.shape) < 1:
        raise ValueError(f"batch_norm_act: x must be (B, C, T) or (B, C) with no empty dimension, got {tuple(x.shape)}")
    C = x.shape[1]
    for name, t in tensors[1:5]:
        if t is not None and tuple(t.shape) != (C,):
            raise ValueError(f"batch_norm_act: {name} must be ({C},), got {tuple(t.shape)}")
    if residual is not None and residual.shape != x.shape:
        raise ValueError(f"batch_norm_act: residual must have x's shape {tuple(x.shape)}, got {tuple(residual.shape)}")
    if (running_mean is None) != (running_var is None):
        raise ValueError("batch_norm_act: running_mean and running_var: both or neither")
    if num_batches_tracked is not None and (not num_batches_tracked.is_cuda or num_batches_tracked.dtype != torch.int64
                                            or num_batches_tracked.numel() != 1 or num_batches_tracked.device != x.device):
        raise ValueError("batch_norm_act: num_batches_tracked must be one int64 on x's device")
    if not training and running_mean is None:
        raise ValueError("batch_norm_act: eval statistics need running_mean and running_var")
    if training and x.numel() // C < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    if training and momentum is None and running_mean is not None and num_batches_tracked is None:
        raise ValueError("batch_norm_act: momentum=None needs num_batches_tracked")
    return _BatchNormAct.apply(x, weight, bias, residual, running_mean, running_var, num_batches_tracked, bool(training), momentum, eps,
                               bool(relu))


class DeviceBatchNorm1d(nn.BatchNorm1d):
    """An ``nn.BatchNorm1d`` -- the same constructor, parameters, buffers and state-dict keys -- whose
    ``forward(x, residual=None, relu=False)`` is ``relu(bn(x) + residual)``: by the device call for float32 device tensors, by
    torch's own statements otherwise (on the CPU it is bit for bit what the blocks compute without it)."""

    @classmethod
    def sharing(cls, bn: nn.BatchNorm1d) -> "DeviceBatchNorm1d":
        """A DeviceBatchNorm1d over the very parameter and buffer objects of ``bn``."""
        new = cls(bn.num_features, eps=bn.eps, momentum=bn.momentum, affine=bn.affine, track_running_stats=bn.track_running_stats)
        if bn.affine:
            new.weight = bn.weight
            new.bias = bn.bias
        if bn.track_running_stats:
            for name in ("running_mean", "running_var", "num_batches_tracked"):
                new._buffers[name] = bn._buffers[name]
        new.train(bn.training)
        return new

    def _on_device(self, x: torch.Tensor, residual: Optional[torch.Tensor]) -> bool:
        """float32 device tensors of the module's width, the module on the same device (a module's parameters and buffers move
        together: the weight and the running mean stand for them)."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() in (2, 3) and x.numel() > 0
                and x.shape[1] == self.num_features):
            return False
        for t in (residual, self.weight, self.running_mean):
            if t is not None and (t.dtype != torch.float32 or t.device != x.device):
                return False
        return residual is None or residual.shape == x.shape

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
        if self._on_device(x, residual):
            # nn.BatchNorm1d.forward's choice of the statistics: the batch's in training and wherever there are no buffers
            batch_stats = self.training or self.running_mean is None
            if batch_stats and x.numel() // x.shape[1] < 2:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
            return _BatchNormAct.apply(x, self.weight, self.bias, residual, self.running_mean, self.running_var,
                                       self.num_batches_tracked, batch_stats, self.momentum, self.eps, relu)
        y = super().forward(x)
        if residual is not None:
            y = y + residual
        return F.relu(y) if relu else y


def use_device_batchnorms(module: nn.Module) -> int:
    """Replace every ``nn.BatchNorm1d`` below ``module`` by a ``DeviceBatchNorm1d`` that shares its parameter and buffer
    objects, so optimisers built before the swap and state dicts stay valid, and set ``fused_norm = True`` on this package's
    own ``DsCnnBlock``, ``DSDilatedConv1d`` and ``TCNBlock``, which then hand their ReLU and residual add to the
    normalisation's call.  Modules that are ``DeviceBatchNorm1d``s already are left alone.  Returns the number swapped."""
    from wekws_amd.model import mdtc, tcn
    swapped = _device.swap_children(
        module, lambda child: not isinstance(child, DeviceBatchNorm1d) and isinstance(child, nn.BatchNorm1d), DeviceBatchNorm1d.sharing)
    for block in module.modules():
        if isinstance(block, (tcn.DsCnnBlock, mdtc.DSDilatedConv1d, mdtc.TCNBlock)):
            block.fused_norm = True
    return swapped
