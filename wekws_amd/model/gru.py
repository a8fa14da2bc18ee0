"""A trainable GRU whose recurrence runs on the device: ``gru_scan`` is the time loop of one layer of ``torch.nn.GRU`` and its
backward through time as two persistent HIP kernels (csrc/gru_train.hip.h) -- one launch each where torch makes
several per step.  The input product ``gi = W_ih x + b_ih`` and the weight, bias and input gradients are large GEMMs and column
sums; they stay torch's (rocBLAS) unless ``device_weight_grads`` is on, which hands the weight and bias gradients -- products
over all ``B T`` rows -- to the split-K kernels of ``wekws_amd.model.linear``.

``DeviceGRU`` is an ``nn.GRU``: the same constructor, parameter names and state-dict keys, so state dicts go both ways (and into
the packed inference model, ``wekws_amd.model.kws_model``).  ``use_device_grus(module)`` swaps the eligible ``nn.GRU`` children of
any module -- the reference's own ``KWSModel`` included -- for ``DeviceGRU``s over the same Parameter objects.

The device path runs for float32 device tensors, ``batch_first=True``, one direction, ``dropout == 0`` and a hidden size the
kernels are built for; everything else -- CPU tensors, other dtypes, packed sequences, 2-D input -- is ``nn.GRU.forward``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from wekws_amd import _capi, _device

MIN_HIDDEN = 16        # csrc/gru_train_plan.h: the built hidden sizes are the multiples of 16 up to 128
MAX_HIDDEN = 128


def in_device_limits(hidden_size) -> bool:
    """The limits of csrc/gru_train_plan.h on the hidden size."""
    try:
        hidden_size = int(hidden_size)
    except (TypeError, ValueError):
        return False
    return hidden_size % 16 == 0 and MIN_HIDDEN <= hidden_size <= MAX_HIDDEN


class _GruScan(torch.autograd.Function):

    @staticmethod
    def forward(ctx, gi, w_hh, b_hh, h0, device_weight_grads=False):
        ctx.device_weight_grads = bool(device_weight_grads)
        B, T, H3 = gi.shape
        H = H3 // 3
        gi, w = gi.contiguous(), w_hh.contiguous()
        b = None if b_hh is None else b_hh.contiguous()
        h = None if h0 is None else h0.contiguous()
        wanted = any(ctx.needs_input_grad)
        y = torch.empty((B, T, H), dtype=gi.dtype, device=gi.device)
        hn = torch.empty((B, H), dtype=gi.dtype, device=gi.device)
        reserve = torch.empty((B, T, 4 * H), dtype=gi.dtype, device=gi.device) if wanted else None
        ptr = _device.ptr
        with _device.on(gi.device):
            _capi.check(_capi.load().wekws_hip_gru_scan_forward(gi.data_ptr(), w.data_ptr(), ptr(b), ptr(h), B, T, H, y.data_ptr(),
                                                                hn.data_ptr(), ptr(reserve), _device.stream(gi.device)),
                        "wekws_hip_gru_scan_forward")
        if wanted:
            ctx.save_for_backward(y, reserve, w, h)
            ctx.set_materialize_grads(False)
        return y, hn

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y, grad_hn):
        want_gi, want_w, want_b, want_h0 = ctx.needs_input_grad[:4]
        if grad_y is None and grad_hn is None:
            return None, None, None, None, None
        y, reserve, w, h0 = ctx.saved_tensors
        B, T, H = y.shape
        gy = None if grad_y is None else grad_y.contiguous()
        ghn = None if grad_hn is None else grad_hn.contiguous()
        dgi = torch.empty((B, T, 3 * H), dtype=y.dtype, device=y.device)
        dgh = torch.empty_like(dgi)
        dh0 = torch.empty((B, H), dtype=y.dtype, device=y.device) if (want_h0 and h0 is not None) else None
        ptr = _device.ptr
        with _device.on(y.device):
            _capi.check(_capi.load().wekws_hip_gru_scan_backward(ptr(gy), ptr(ghn), y.data_ptr(), ptr(h0), reserve.data_ptr(),
                                                                 w.data_ptr(), B, T, H, dgi.data_ptr(), dgh.data_ptr(), ptr(dh0),
                                                                 _device.stream(y.device)), "wekws_hip_gru_scan_backward")
        dw = db = None
        if ctx.device_weight_grads and (want_w or want_b):
            from wekws_amd.model.linear import _weight_grad
            g2 = dgh.view(B * T, 3 * H)
            if want_w:
                h_prev = torch.empty_like(y)
                h_prev[:, 1:] = y[:, :-1]
                if h0 is None:
                    h_prev[:, 0].zero_()
                else:
                    h_prev[:, 0] = h0
                dw, db = _weight_grad(h_prev.view(B * T, H), g2, True, want_b)
            else:
                _, db = _weight_grad(g2, g2, False, True)          # x is not read without grad_w
            return dgi if want_gi else None, dw, db, dh0, None
        if want_w:
            # dW_hh = dgh^T h_prev over all (b, t): h_prev[t] = y[t-1], h_prev[0] = h0
            h_prev = torch.empty_like(y)
            h_prev[:, 1:] = y[:, :-1]
            if h0 is None:
                h_prev[:, 0].zero_()
            else:
                h_prev[:, 0] = h0
            dw = dgh.view(B * T, 3 * H).t().mm(h_prev.view(B * T, H))
        if want_b:
            db = dgh.view(B * T, 3 * H).sum(0)
        return dgi if want_gi else None, dw, db, dh0, None


def gru_scan(gi: torch.Tensor, w_hh: torch.Tensor, b_hh: Optional[torch.Tensor], h0: Optional[torch.Tensor] = None,
             device_weight_grads: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """The recurrence of one GRU layer on the device, differentiable once: ``gi`` (B, T, 3H) float32 on a ROCm device, the input
    product ``W_ih x + b_ih`` in PyTorch's gate order r, z, n; ``w_hh`` (3H, H); ``b_hh`` (3H) or None; ``h0`` (B, H) or None for
    zeros.  Returns ``(y, hn)``: every step's hidden state (B, T, H) and the last one (B, H).  One launch forward and one backward,
    on the current stream; nothing is read on the host, and only the gradients autograd asks for are computed.  The gradients of
    ``w_hh`` and ``b_hh`` are torch's ``mm`` and ``sum`` over the scan's ``dgh``; with ``device_weight_grads`` they are
    ``wekws_amd.model.linear``'s split-K kernels.  No CPU fallback: anything else raises."""
    tensors = [("gi", gi), ("w_hh", w_hh)] + ([("b_hh", b_hh)] if b_hh is not None else []) + ([("h0", h0)] if h0 is not None else [])
    _device.require_float32("gru_scan", gi, tensors)
    if gi.dim() != 3 or min(gi.shape) < 1 or gi.shape[2] % 3:
        raise ValueError(f"gru_scan: gi must be (B, T, 3H) with no empty dimension, got {tuple(gi.shape)}")
    B, _, H3 = gi.shape
    H = H3 // 3
    if not in_device_limits(H):
        raise ValueError(f"gru_scan: H={H} outside the kernels' limits (a multiple of 16 within {MIN_HIDDEN} .. {MAX_HIDDEN})")
    if tuple(w_hh.shape) != (H3, H):
        raise ValueError(f"gru_scan: w_hh must be ({H3}, {H}), got {tuple(w_hh.shape)}")
    if b_hh is not None and tuple(b_hh.shape) != (H3,):
        raise ValueError(f"gru_scan: b_hh must be ({H3},), got {tuple(b_hh.shape)}")
    if h0 is not None and tuple(h0.shape) != (B, H):
        raise ValueError(f"gru_scan: h0 must be ({B}, {H}), got {tuple(h0.shape)}")
    return _GruScan.apply(gi, w_hh, b_hh, h0, bool(device_weight_grads))


class DeviceGRU(nn.GRU):
    """``torch.nn.GRU`` whose recurrence runs in ``gru_scan``: per layer one ``torch.addmm`` for ``gi``, then the scan.
    ``forward(x, hx=None) -> (output, h_n)`` with nn.GRU's shapes; an ``hx`` with zero elements means zeros, as the packed model
    treats the reference's empty ``in_cache``.  The device path never calls ``flatten_parameters``, so the parameters may be views
    of an optimiser's flat buffers (``wekws_amd.optim.ClipAdam``).  ``device_weight_grads`` (off by default; turned on by
    ``wekws_amd.model.linear.use_device_weight_grads``) takes all four parameter gradients of a layer from the split-K kernels of
    ``wekws_amd.model.linear`` instead of rocBLAS."""

    device_weight_grads = False            # (the class's default: a module unpickled from before the switch has it off)

    def __init__(self, *args, device_weight_grads: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.device_weight_grads = bool(device_weight_grads)

    @classmethod
    def sharing(cls, gru: nn.GRU) -> "DeviceGRU":
        """A DeviceGRU over the very Parameter objects of ``gru``."""
        p = gru.weight_hh_l0
        new = cls(gru.input_size, gru.hidden_size, num_layers=gru.num_layers, bias=gru.bias, batch_first=gru.batch_first,
                  dropout=gru.dropout, bidirectional=gru.bidirectional, device=p.device, dtype=p.dtype)
        for name, param in gru.named_parameters(recurse=False):
            setattr(new, name, param)
        new.device_weight_grads = bool(getattr(gru, "device_weight_grads", False))
        new.train(gru.training)
        return new

    def _on_device(self, x, hx) -> bool:
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.numel() > 0
                and _eligible(self)):
            return False
        if hx is not None and hx.numel() > 0 and not (hx.is_cuda and hx.dtype == torch.float32 and hx.device == x.device):
            return False
        return all(p.is_cuda and p.dtype == torch.float32 and p.device == x.device for p in self.parameters(recurse=False))

    def forward(self, input, hx=None):  # noqa: A002 (nn.GRU's own argument names)
        if not self._on_device(input, hx):
            return super().forward(input, hx)
        B, T, _ = input.shape
        H, L = self.hidden_size, self.num_layers
        if hx is not None and hx.numel() == 0:
            hx = None
        if hx is not None and tuple(hx.shape) != (L, B, H):
            raise RuntimeError(f"Expected hidden size {(L, B, H)}, got {list(hx.shape)}")
        x, last = input, []
        for layer in range(L):
            w_ih, w_hh = getattr(self, f"weight_ih_l{layer}"), getattr(self, f"weight_hh_l{layer}")
            b_ih = getattr(self, f"bias_ih_l{layer}") if self.bias else None
            b_hh = getattr(self, f"bias_hh_l{layer}") if self.bias else None
            flat = x.reshape(B * T, x.shape[2])
            if self.device_weight_grads:
                from wekws_amd.model.linear import linear
                gi = linear(flat, w_ih, b_ih)
            else:
                gi = torch.addmm(b_ih, flat, w_ih.t()) if b_ih is not None else flat.mm(w_ih.t())
            x, hn = gru_scan(gi.view(B, T, 3 * H), w_hh, b_hh, None if hx is None else hx[layer], self.device_weight_grads)
            last.append(hn)
        return x, torch.stack(last, 0)


def _eligible(gru: nn.GRU) -> bool:
    """What the device path needs of a module, whatever it is given: batch-first, one direction, no dropout, a built hidden size."""
    return (gru.batch_first and not gru.bidirectional and float(gru.dropout) == 0.0 and getattr(gru, "proj_size", 0) == 0
            and in_device_limits(gru.hidden_size))


def use_device_grus(module: nn.Module) -> int:
    """Replace every eligible ``nn.GRU`` child below ``module`` -- ``batch_first``, one direction, no dropout, a hidden size the
    kernels are built for -- by a ``DeviceGRU`` that shares its Parameter objects, so optimisers built before the swap and state
    dicts stay valid.  Other GRUs, and ``DeviceGRU``s, are left alone.  Returns the number swapped."""
    return _device.swap_children(
        module, lambda child: not isinstance(child, DeviceGRU) and isinstance(child, nn.GRU) and _eligible(child), DeviceGRU.sharing)
