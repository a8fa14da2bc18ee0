"""How a training layer's wrapper reaches its C entry point, and how a module is swapped for its device twin: the host plumbing
of ``wekws_amd.model.{fsmn,depthwise,batchnorm,gru,linear,pointwise}``, written down once.  Imports no layer
module, so importing one layer never loads another.
"""
from __future__ import annotations

import contextlib
import ctypes

import torch

from wekws_amd import _capi


def stream(device) -> ctypes.c_void_p:
    """The current stream of ``device`` as the C entry points take it."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t: torch.Tensor | None):
    """A tensor's address, None (NULL) for no tensor."""
    return t.data_ptr() if t is not None else None


_NO_GUARD = contextlib.nullcontext()


def on(device: torch.device):
    """The device made current for a call, when it is not already (the step's hot path: one comparison)."""
    return _NO_GUARD if torch.cuda.current_device() == device.index else torch.cuda.device(device)


_workspaces: dict[torch.device, torch.Tensor] = {}


def workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """The one ``uint8`` scratch buffer of a device, of at least ``nbytes`` bytes, grown on demand and shared by every layer
    that takes its workspace from here (the FSMN memory block, the depthwise Conv1d, BatchNorm1d).  Sharing is legal on one
    condition, which those entry points keep: every byte a C call writes to its workspace is consumed by launches enqueued in
    that same call -- tile partials by the fold that follows them, BatchNorm's ``tracked_before`` and ``coef`` likewise -- so a
    call expects nothing of the buffer's contents and leaves nothing in it for a later one.  A layer that kept workspace
    contents across calls would need a buffer of its own.  Calls on one stream are ordered, so they may share it; a caller that
    runs these layers on several streams at once -- different layers as much as the same one -- serialises them itself."""
    ws = _workspaces.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        _workspaces[device] = ws
    return ws


_library_bytes: dict[tuple[str, tuple], int] = {}


def library_bytes(sizer: str, shape: tuple, error: type, what: str | None = None) -> int:
    """``lib.<sizer>(*shape)``: a workspace size, asked of the library once per shape.  A size of 0 is the library's refusal
    and raises ``error`` -- the calling layer's own exception type -- with the library's text, prefixed by ``what`` (the
    sizer's name when not given).  The cache is one dict for the process and is never emptied: an entry (a few hundred bytes)
    per distinct shape a run meets, which a run with many distinct (B, T) grows accordingly."""
    nbytes = _library_bytes.get((sizer, shape))
    if nbytes is None:
        nbytes = int(getattr(_capi.load(), sizer)(*shape))
        if nbytes == 0:
            raise error(f"{what or sizer}: {_capi.last_error()}")
        _library_bytes[(sizer, shape)] = nbytes
    return nbytes


def require_float32(op: str, first: torch.Tensor, named_tensors) -> None:
    """Every ``(name, tensor)`` is a float32 tensor on a ROCm device, and on the device of ``first``; ``ValueError`` naming the
    first that is not.  Shape checks stay with each layer."""
    for name, t in named_tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise ValueError(f"{op}: {name} must be a float32 tensor on a ROCm device (no CPU fallback)")
        if t.device != first.device:
            raise ValueError(f"{op}: tensors on one device, got {first.device} and {t.device}")


def swap_children(module: torch.nn.Module, wanted, make) -> int:
    """Replace every child below ``module`` for which ``wanted(child)`` holds by ``make(child)``.  Both walks are over
    snapshots, so a replacement is never visited.  Returns the number replaced."""
    swapped = 0
    for parent in list(module.modules()):
        for name, child in list(parent.named_children()):
            if wanted(child):
                setattr(parent, name, make(child))
                swapped += 1
    return swapped
