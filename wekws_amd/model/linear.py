"""Linear layers whose weight and bias gradients are computed on the device by the package's own kernels:
``dW (O, I) = g^T x`` and ``db (O) = sum_r g`` over the ``R = B T`` rows of a batch, as a split-K product with a stated
arithmetic -- float32 chains of 512 rows on the matrix cores, added and folded in double, rounded once (csrc/linear_wgrad_plan.h,
csrc/linear_wgrad.hip.h) -- so their bits are a function of the inputs and the shape.  The forward ``x W^T + b``
and the input gradient ``g W`` are large regular GEMMs and stay torch's, bit for bit.

``DeviceLinear`` is an ``nn.Linear``: the same constructor, parameters and state-dict keys.  ``use_device_weight_grads(module)``
swaps every ``nn.Linear`` below a module -- this package's and the reference's own -- for a ``DeviceLinear`` over the same
Parameter objects and turns on the same path for the weight gradients of every ``DeviceGRU``.

The device path runs for float32 tensors on a ROCm device with at least one row; everything else is ``nn.Linear.forward``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from wekws_amd import _capi, _device

MAX_FEATURES = 65535        # csrc/linear_wgrad_plan.h: O and I


def _weight_grad(x2: torch.Tensor, g2: torch.Tensor, want_w: bool, want_b: bool):
    """x2 (R, I), g2 (R, O): float32, contiguous, on one ROCm device; at least one of the two is wanted."""
    R, I = x2.shape
    O = g2.shape[1]
    nbytes = _device.library_bytes("wekws_hip_linear_wgrad_workspace_bytes", (R, O, I), ValueError, "linear_weight_grad")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x2.device)
    dw = torch.empty((O, I), dtype=torch.float32, device=x2.device) if want_w else None
    db = torch.empty((O,), dtype=torch.float32, device=x2.device) if want_b else None
    with _device.on(x2.device):
        _capi.check(_capi.load().wekws_hip_linear_wgrad(x2.data_ptr(), g2.data_ptr(), R, O, I, _device.ptr(dw), _device.ptr(db),
                                                        ws.data_ptr(), nbytes, _device.stream(x2.device)), "wekws_hip_linear_wgrad")
    return dw, db


def _check_pair(x, g):
    _device.require_float32("linear_weight_grad", x, (("x", x), ("g", g)))
    if x.dim() < 1 or g.dim() != x.dim() or x.shape[:-1] != g.shape[:-1]:
        raise ValueError(f"linear_weight_grad: x (..., I) and g (..., O) with the same leading dimensions, got {tuple(x.shape)} "
                         f"and {tuple(g.shape)}")
    I, O = x.shape[-1], g.shape[-1]
    R = x.numel() // I if I else 0
    if R < 1 or not 1 <= I <= MAX_FEATURES or not 1 <= O <= MAX_FEATURES:
        raise ValueError(f"linear_weight_grad: at least one row and 1 .. {MAX_FEATURES} features, got R={R} O={O} I={I}")
    return R, O, I


def linear_weight_grad(x: torch.Tensor, g: torch.Tensor, want_bias: bool = True
                       ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The gradients of ``y = x W^T + b`` with respect to ``W`` and ``b``: ``x`` (..., I) and ``g`` (..., O), float32 on a ROCm
    device, the leading dimensions flattened to R rows.  Returns ``(dW (O, I), db (O) or None)``.  Two launches on the current
    stream and one workspace from ``torch.empty``; nothing is read on the host.  No CPU fallback: anything else raises."""
    R, O, I = _check_pair(x, g)
    return _weight_grad(x.reshape(R, I).contiguous(), g.reshape(R, O).contiguous(), True, bool(want_bias))


class _Linear(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return F.linear(x, weight, bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        want_x, want_w, want_b = ctx.needs_input_grad
        dx = g.matmul(weight) if want_x else None
        dw = db = None
        if want_w or want_b:
            I, O = x.shape[-1], weight.shape[0]
            dw, db = _weight_grad(x.reshape(-1, I).contiguous(), g.reshape(-1, O).contiguous(), want_w, want_b)
        return dx, dw, db


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.linear`` whose weight and bias gradients come from ``linear_weight_grad``'s kernels, differentiable once: ``x``
    (..., I), ``weight`` (O, I), ``bias`` (O) or None, float32 on one ROCm device, at least one row.  The forward is
    ``F.linear`` and the input gradient ``g.matmul(weight)``, both torch's bit for bit; only the gradients autograd asks for are
    computed.  No CPU fallback: anything else raises."""
    tensors = [("x", x), ("weight", weight)] + ([("bias", bias)] if bias is not None else [])
    _device.require_float32("linear", x, tensors)
    if weight.dim() != 2 or x.dim() < 1 or x.shape[-1] != weight.shape[1] or x.numel() == 0:
        raise ValueError(f"linear: x (..., I) with at least one row and weight (O, I), got {tuple(x.shape)} and {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"linear: bias must be ({weight.shape[0]},), got {tuple(bias.shape)}")
    if not (1 <= weight.shape[0] <= MAX_FEATURES and 1 <= weight.shape[1] <= MAX_FEATURES):
        raise ValueError(f"linear: 1 .. {MAX_FEATURES} features, got weight {tuple(weight.shape)}")
    return _Linear.apply(x, weight, bias)


class DeviceLinear(nn.Linear):
    """``torch.nn.Linear`` whose weight and bias gradients come from ``linear``: the same constructor, parameters and state-dict
    keys.  The parameters may be views of an optimiser's flat buffers (``wekws_amd.optim.ClipAdam``)."""

    @classmethod
    def sharing(cls, lin: nn.Linear) -> "DeviceLinear":
        """A DeviceLinear over the very Parameter objects of ``lin``."""
        new = cls(lin.in_features, lin.out_features, bias=lin.bias is not None, device="meta")
        new.weight = lin.weight
        if lin.bias is not None:
            new.bias = lin.bias
        new.train(lin.training)
        return new

    def _on_device(self, x) -> bool:
        w, b = self.weight, self.bias
        return (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() >= 1 and x.numel() > 0
                and x.shape[-1] == self.in_features and w.is_cuda and w.dtype == torch.float32 and w.device == x.device
                and (b is None or (b.is_cuda and b.dtype == torch.float32 and b.device == x.device))
                and 1 <= self.in_features <= MAX_FEATURES and 1 <= self.out_features <= MAX_FEATURES)

    def forward(self, input):  # noqa: A002 (nn.Linear's own argument name)
        if not self._on_device(input):
            return super().forward(input)
        return linear(input, self.weight, self.bias)


def use_device_weight_grads(module: nn.Module) -> int:
    """Replace every ``nn.Linear`` child below ``module`` by a ``DeviceLinear`` that shares its Parameter objects, and turn
    ``device_weight_grads`` on for every ``DeviceGRU``, so optimisers built before the swap and state dicts stay valid.
    Idempotent: what is changed already is left alone.  Returns the number of modules changed."""
    from wekws_amd.model.gru import DeviceGRU
    # (exactly nn.Linear: a subclass with a forward of its own keeps it)
    changed = _device.swap_children(module, lambda child: type(child) is nn.Linear, DeviceLinear.sharing)
    for m in module.modules():
        if isinstance(m, DeviceGRU) and not m.device_weight_grads:
            m.device_weight_grads = True
            changed += 1
    return changed
