"""A trainable FSMN whose memory blocks run on the device: ``fsmn_memory`` is the reference's ``FSMNBlock.forward`` with an
empty cache (wekws/model/fsmn.py:214-253) and its autograd as three HIP kernels (csrc/fsmn_memory.hip.h) -- a
causal sparse FIR per channel, its mirror image for the input gradient, and a fixed-order double sum for the tap gradients.

``FSMNBlock`` and ``FSMN`` mirror the reference's modules: the same constructors, parameter names and shapes, so state dicts go
both ways (and into the packed inference model, ``wekws_amd.model.kws_model``).  The Linear layers stay torch's.
``use_device_memory_blocks(module)`` swaps the memory blocks of any module -- the reference's own ``FSMN`` or ``KWSModel``
included -- for ``FSMNBlock``s that share their parameter objects.

The device call runs for float32 device tensors with an empty cache and parameters inside the kernels' limits; a non-empty
cache (streaming), CPU tensors and other dtypes take torch's own ops, statement by statement what the reference does.
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from wekws_amd import _capi, _device

MAX_TAPS = 32          # lorder + rorder                         (csrc/fsmn_memory_plan.h)
MAX_WINDOW = 256       # rorder * rstride + (lorder - 1) * lstride + 1


def in_device_limits(lorder, rorder, lstride, rstride) -> bool:
    """The limits of csrc/fsmn_memory_plan.h on a block's parameters."""
    try:
        lorder, rorder, lstride, rstride = int(lorder), int(rorder), int(lstride), int(rstride)
    except (TypeError, ValueError):
        return False
    return (lorder >= 1 and rorder >= 1 and lstride >= 1 and rstride >= 1 and lorder + rorder <= MAX_TAPS
            and rorder * rstride + (lorder - 1) * lstride + 1 <= MAX_WINDOW)


class _FsmnMemory(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, w_left, w_right, lstride, rstride):
        B, T, D = x.shape
        lorder, rorder = w_left.numel() // D, w_right.numel() // D
        x, wl, wr = x.contiguous(), w_left.contiguous(), w_right.contiguous()
        y = torch.empty_like(x)
        with _device.on(x.device):
            _capi.check(_capi.load().wekws_hip_fsmn_memory_forward(x.data_ptr(), B, T, D, wl.data_ptr(), lorder, lstride, wr.data_ptr(),
                                                                   rorder, rstride, y.data_ptr(), _device.stream(x.device)),
                        "wekws_hip_fsmn_memory_forward")
        ctx.save_for_backward(x, wl, wr)
        ctx.strides = (lstride, rstride)
        ctx.w_shapes = (w_left.shape, w_right.shape)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, wl, wr = ctx.saved_tensors
        lstride, rstride = ctx.strides
        B, T, D = x.shape
        lorder, rorder = wl.numel() // D, wr.numel() // D
        want_x = ctx.needs_input_grad[0]
        want_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not (want_x or want_w):
            return None, None, None, None, None
        g = grad_y.contiguous()
        lib = _capi.load()
        dx = torch.empty_like(x) if want_x else None
        dwl = torch.empty_like(wl) if want_w else None
        dwr = torch.empty_like(wr) if want_w else None
        ws, ws_bytes = None, 0
        if want_w:
            ws_bytes = _device.library_bytes("wekws_hip_fsmn_memory_workspace_bytes", (B, T, D, lorder, rorder), _capi.HipLibraryError)
            ws = _device.workspace(x.device, ws_bytes)
        with _device.on(x.device):
            _capi.check(lib.wekws_hip_fsmn_memory_backward(
                x.data_ptr(), g.data_ptr(), B, T, D, wl.data_ptr(), lorder, lstride, wr.data_ptr(), rorder, rstride,
                _device.ptr(dx), _device.ptr(dwl), _device.ptr(dwr), _device.ptr(ws), ws_bytes, _device.stream(x.device)),
                "wekws_hip_fsmn_memory_backward")
        lshape, rshape = ctx.w_shapes
        return (dx, dwl.view(lshape) if ctx.needs_input_grad[1] else None, dwr.view(rshape) if ctx.needs_input_grad[2] else None,
                None, None)


def fsmn_memory(x: torch.Tensor, w_left: torch.Tensor, w_right: torch.Tensor, lstride: int = 1, rstride: int = 1) -> torch.Tensor:
    """The memory block of an FSMN unit on the device, differentiable once: ``x`` (B, T, D) float32 on a ROCm device, ``w_left``
    of D * lorder elements laid out (D, lorder) -- ``conv_left.weight`` (D, 1, lorder, 1) as it is -- and ``w_right`` likewise.
    Returns y (B, T, D): the reference block's output for an empty cache.  Non-contiguous inputs are made contiguous; the call
    runs on the current stream and reads nothing on the host.  No CPU fallback: anything else raises."""
    _device.require_float32("fsmn_memory", x, (("x", x), ("w_left", w_left), ("w_right", w_right)))
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError(f"fsmn_memory: x must be (B, T, D) with no empty dimension, got {tuple(x.shape)}")
    D = x.shape[2]
    for name, w in (("w_left", w_left), ("w_right", w_right)):
        if w.dim() < 2 or w.shape[0] != D or w.numel() == 0:
            raise ValueError(f"fsmn_memory: {name} must be (D, order) or (D, 1, order, 1) with D = {D}, got {tuple(w.shape)}")
    lorder, rorder = w_left.numel() // D, w_right.numel() // D
    if not in_device_limits(lorder, rorder, lstride, rstride):
        raise ValueError(f"fsmn_memory: lorder={lorder} rorder={rorder} lstride={lstride} rstride={rstride} outside the kernels' "
                         f"limits (orders and strides >= 1, at most {MAX_TAPS} taps, a window of at most {MAX_WINDOW} frames)")
    return _FsmnMemory.apply(x, w_left, w_right, int(lstride), int(rstride))


def _empty_cache() -> torch.Tensor:
    return torch.zeros(0, 0, 0, 0, dtype=torch.float)


def _split(input):
    """The reference's modules pass (tensor, cache) pairs along an nn.Sequential; a bare tensor gets an empty cache."""
    if isinstance(input, tuple):
        return input
    return input, _empty_cache()


class LinearTransform(nn.Module):

    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.linear = nn.Linear(input_dim, output_dim, bias=False)

    def forward(self, input):
        x, cache = _split(input)
        return self.linear(x), cache


class AffineTransform(nn.Module):

    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.linear = nn.Linear(input_dim, output_dim)

    def forward(self, input):
        x, cache = _split(input)
        return self.linear(x), cache


class RectifiedLinear(nn.Module):

    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.dim = input_dim
        self.relu = nn.ReLU()
        self.dropout = nn.Dropout(0.1)          # as in the reference: constructed, never applied

    def forward(self, input):
        x, cache = _split(input)
        return self.relu(x), cache


class FSMNBlock(nn.Module):
    """The reference's memory block: depthwise ``conv_left`` (D, 1, lorder, 1) over the past and ``conv_right``
    (D, 1, rorder, 1) over the next ``rorder * rstride`` frames, plus the delayed input itself.
    ``forward((input, in_cache)) -> (output, out_cache)``."""

    def __init__(self, input_dim: int, output_dim: int, lorder=None, rorder=None, lstride=1, rstride=1):
        super().__init__()
        self.dim = input_dim
        if lorder is None:
            return
        self.lorder = lorder
        self.rorder = rorder
        self.lstride = lstride
        self.rstride = rstride
        self.conv_left = nn.Conv2d(self.dim, self.dim, [lorder, 1], dilation=[lstride, 1], groups=self.dim, bias=False)
        if rorder > 0:
            self.conv_right = nn.Conv2d(self.dim, self.dim, [rorder, 1], dilation=[rstride, 1], groups=self.dim, bias=False)
        else:
            self.conv_right = None

    @classmethod
    def sharing(cls, block: nn.Module) -> "FSMNBlock":
        """An FSMNBlock over the very parameter objects of ``block`` (anything with conv_left, conv_right, lorder, rorder,
        lstride, rstride)."""
        new = cls(block.conv_left.weight.shape[0], block.conv_left.weight.shape[0])
        new.lorder, new.rorder, new.lstride, new.rstride = block.lorder, block.rorder, block.lstride, block.rstride
        new.conv_left = block.conv_left
        new.conv_right = block.conv_right
        new.train(block.training)
        return new

    def _on_device(self, x: torch.Tensor, in_cache) -> bool:
        return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.numel() > 0
                and (in_cache is None or len(in_cache) == 0) and self.conv_right is not None
                and self.conv_left.weight.is_cuda and self.conv_left.weight.dtype == torch.float32
                and self.conv_right.weight.dtype == torch.float32
                and in_device_limits(self.lorder, self.rorder, self.lstride, self.rstride))

    def forward(self, input):
        x, in_cache = _split(input)
        pad = (self.lorder - 1) * self.lstride + self.rorder * self.rstride
        if self._on_device(x, in_cache):
            y = fsmn_memory(x, self.conv_left.weight, self.conv_right.weight, self.lstride, self.rstride)
            # the reference's out_cache: the last `pad` frames of the left-padded input as (B, D, pad, 1)
            x_per = x.unsqueeze(1).permute(0, 3, 2, 1)
            out_cache = F.pad(x_per, [0, 0, pad, 0])[:, :, -pad:, :]
            return y, out_cache
        return self._forward_torch(x, in_cache, pad)

    def _forward_torch(self, x, in_cache, pad):
        """torch's own ops, as the reference has them: (B, T, D) -> (B, D, T, 1), left padding or the cache in front, the two
        grouped convolutions over their slices, the delayed input added."""
        right = self.rorder * self.rstride
        x_per = x.unsqueeze(1).permute(0, 3, 2, 1)
        if in_cache is None or len(in_cache) == 0:
            x_pad = F.pad(x_per, [0, 0, pad, 0])
        else:
            x_pad = torch.cat((in_cache.to(x_per.device), x_per), dim=2)
        out_cache = x_pad[:, :, -pad:, :]
        out = x_pad[:, :, (self.lorder - 1) * self.lstride:-right, :] + self.conv_left(x_pad[:, :, :-right, :])
        if self.conv_right is not None:
            y_right = x_pad[:, :, -(x_per.size(2) + right):, :][:, :, self.rstride:, :]
            out = out + self.conv_right(y_right)
        return out.permute(0, 3, 2, 1).squeeze(1), out_cache


def _build_repeats(fsmn_layers, linear_dim, proj_dim, lorder, rorder, lstride=1, rstride=1):
    # (the reference builds its units with strides 1, 1 whatever it is given: wekws/model/fsmn.py:392)
    return nn.Sequential(*[
        nn.Sequential(LinearTransform(linear_dim, proj_dim), FSMNBlock(proj_dim, proj_dim, lorder, rorder, 1, 1),
                      AffineTransform(proj_dim, linear_dim), RectifiedLinear(linear_dim, linear_dim)) for _ in range(fsmn_layers)
    ])


class FSMN(nn.Module):
    """wekws/model/fsmn.py::FSMN without the Kaldi text I/O and the quantisation stubs: the same constructor arguments, the
    same state-dict keys, ``forward(input, in_cache) -> (logits, cache)``."""

    def __init__(self, input_dim: int, input_affine_dim: int, fsmn_layers: int, linear_dim: int, proj_dim: int, lorder: int,
                 rorder: int, lstride: int, rstride: int, output_affine_dim: int, output_dim: int):
        super().__init__()
        self.input_dim = input_dim
        self.input_affine_dim = input_affine_dim
        self.fsmn_layers = fsmn_layers
        self.linear_dim = linear_dim
        self.proj_dim = proj_dim
        self.lorder = lorder
        self.rorder = rorder
        self.lstride = lstride
        self.rstride = rstride
        self.output_affine_dim = output_affine_dim
        self.output_dim = output_dim
        self.padding = (lorder - 1) * lstride + rorder * rstride
        self.in_linear1 = AffineTransform(input_dim, input_affine_dim)
        self.in_linear2 = AffineTransform(input_affine_dim, linear_dim)
        self.relu = RectifiedLinear(linear_dim, linear_dim)
        self.fsmn = _build_repeats(fsmn_layers, linear_dim, proj_dim, lorder, rorder, lstride, rstride)
        self.out_linear1 = AffineTransform(linear_dim, output_affine_dim)
        self.out_linear2 = AffineTransform(output_affine_dim, output_dim)

    def forward(self, input: torch.Tensor, in_cache: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """input (B, T, D); in_cache (B, proj_dim, padding, layers) or empty / None -> (logits (B, T, output_dim), cache)."""
        if in_cache is None or len(in_cache) == 0:
            caches = [_empty_cache() for _ in range(len(self.fsmn))]
        else:
            caches = [in_cache[:, :, :, i:i + 1] for i in range(in_cache.size(-1))]
        x, _ = self.relu(self.in_linear2(self.in_linear1((input, caches))))
        for layer, unit in enumerate(self.fsmn):
            x, caches[layer] = unit((x, caches[layer]))
        x, _ = self.out_linear2(self.out_linear1(x))
        return x, torch.cat(caches, dim=-1)


def _is_memory_block(m: nn.Module) -> bool:
    return all(hasattr(m, a) for a in ("conv_left", "conv_right", "lorder", "rorder", "lstride", "rstride"))


def use_device_memory_blocks(module: nn.Module) -> int:
    """Replace every memory block below ``module`` -- recognised by its attributes: conv_left, conv_right, lorder, rorder,
    lstride, rstride -- by an ``FSMNBlock`` that shares its parameter objects, so optimisers built before the swap and state
    dicts stay valid.  Blocks without a right context (``rorder == 0``, which the reference cannot run either) or outside the
    kernels' limits are left alone, and so are blocks that are ``FSMNBlock``s already.  Returns the number swapped."""

    def wanted(child: nn.Module) -> bool:
        if isinstance(child, FSMNBlock) or not _is_memory_block(child):
            return False
        return child.conv_right is not None and in_device_limits(child.lorder, child.rorder, child.lstride, child.rstride)

    return _device.swap_children(module, wanted, FSMNBlock.sharing)
