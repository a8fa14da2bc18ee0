"""The optimiser step on the device: ``ClipAdam`` is ``torch.optim.Adam`` over flat buffers, with the last three statements of
the reference's training step (wekws/utils/executor.py:58-60) as one call that reads nothing on the host::

    grad_norm = clip_grad_norm_(model.parameters(), clip)
    if torch.isfinite(grad_norm):            ->      grad_norm = optimizer.clip_and_step(clip)
        optimizer.step()

through ``wekws_hip_clip_adam_step`` (csrc/optim.hip.h): three small launches over four flat float32 buffers -- params, grads,
exp_avg, exp_avg_sq -- that the optimiser allocates once.  Every parameter's ``.data`` and ``.grad`` are views into the first
two, so the kernels see four base pointers and a length, and autograd accumulates straight into the flat gradient.

Deviations from ``clip_grad_norm_`` + ``optim.Adam``:

1. ``p.grad`` is left unscaled: the reference scales it in place, here the clip coefficient is folded into the update.
2. A parameter autograd never wrote to has gradient 0, not ``None``: it still decays (and its moments still shrink), where
   torch's Adam skips it.  Every parameter of the reference's models is used.
3. The norm is accumulated in double.  A gradient whose float32 sum of squares overflows while its norm is still a finite
   float32 is clipped and stepped, where the reference skips the step.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Sequence, Tuple

import torch

from wekws_amd import _capi

ALIGN_ELEMS = 16          # every tensor's view starts on a multiple of 16 floats (64 bytes) of the flat buffers


class FlatViews:
    """Where each tensor of ``shapes`` lies in a flat buffer, and the bookkeeping that ties parameters to two such buffers.
    Pure tensor plumbing: works on CPU tensors too (tests/test_optim_ref.py)."""

    def __init__(self, shapes: Sequence[Tuple[int, ...]]):
        self.shapes = [tuple(int(d) for d in s) for s in shapes]
        self.numels = [int(math.prod(s)) for s in self.shapes]
        self.offsets: List[int] = []
        at = 0
        for n in self.numels:
            self.offsets.append(at)
            at += (n + ALIGN_ELEMS - 1) // ALIGN_ELEMS * ALIGN_ELEMS
        self.total = max(at, ALIGN_ELEMS)           # the gaps stay zero in every buffer: a zero gradient on a zero parameter

    def views(self, flat: torch.Tensor) -> List[torch.Tensor]:
        assert flat.dim() == 1 and flat.numel() == self.total and flat.is_contiguous()
        return [flat[o:o + n].view(s) for o, n, s in zip(self.offsets, self.numels, self.shapes)]

    def adopt(self, params: Sequence[torch.Tensor], flat_p: torch.Tensor, flat_g: torch.Tensor) -> None:
        """Copy the parameters into ``flat_p``, make every ``p.data`` its view and every ``p.grad`` the view of the zeroed
        ``flat_g``.  Autograd then accumulates into that view in place."""
        flat_g.zero_()
        with torch.no_grad():
            for p, pv, gv in zip(params, self.views(flat_p), self.views(flat_g)):
                pv.copy_(p.data)
                p.data = pv
                p.grad = gv

    def broken(self, params: Sequence[torch.Tensor], flat_p: torch.Tensor, flat_g: torch.Tensor) -> List[str]:
        """What no longer points into the flat buffers, as text; [] when every view is where ``adopt`` put it.  Compares
        addresses on the host: no device work."""
        size = flat_p.element_size()
        base_p, base_g = flat_p.data_ptr(), flat_g.data_ptr()
        bad = []
        for i, (p, o, s) in enumerate(zip(params, self.offsets, self.shapes)):
            if p.data_ptr() != base_p + o * size or tuple(p.shape) != s or not p.is_contiguous():
                bad.append(f"parameter {i} {s}: its data is no longer a view of the flat buffer")
            g = p.grad
            if g is None:
                bad.append(f"parameter {i} {s}: its .grad is None")
            elif g.data_ptr() != base_g + o * size or tuple(g.shape) != s or not g.is_contiguous() or g.dtype != flat_g.dtype:
                bad.append(f"parameter {i} {s}: its .grad is no longer a view of the flat gradient")
        return bad


# byte offsets of the state block (include/wekws_hip.h)
_STATE_BYTES = 64
_I64_STEP, _I64_SKIPPED = 0, 1            # as int64 words
_F32_COEF, _F32_NORM = 10, 11             # as float32 words


class ClipAdam(torch.optim.Optimizer):
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` for exactly one group of float32 parameters on one ROCm
    device, stepping on the device (module docstring).  ``amsgrad``, ``maximize``, several groups, other dtypes and CPU
    tensors raise.

    Construction moves the parameters: each ``p.data`` becomes a view of one flat buffer and each ``p.grad`` a view of a
    second, zeroed one.  Whatever replaces those tensors afterwards -- ``model.to(...)``, ``p.grad = None``,
    ``model.zero_grad(set_to_none=True)`` -- breaks the views; the next step raises RuntimeError rather than step buffers the
    model no longer uses.  Call the optimiser's own ``zero_grad``.

    ``lr`` is read from ``param_groups[0]['lr']`` at every step, so ``ReduceLROnPlateau`` and the other schedulers work
    unchanged.  ``steps``, ``skipped_steps`` and ``last_clip_coef`` are device scalars, views of the state block: they change
    with the next step, and reading them synchronises.  ``state_dict`` / ``load_state_dict`` use ``torch.optim.Adam``'s format
    both ways; ``step`` is one counter for all parameters, and the count of skipped steps is not part of that format."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise ValueError("ClipAdam: amsgrad and maximize are not supported")
        if isinstance(lr, torch.Tensor):
            raise TypeError("ClipAdam: lr must be a Python number (it is passed by value at every step)")
        self._check_hyper(lr, betas, eps, weight_decay)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError(f"ClipAdam: exactly one parameter group, got {len(self.param_groups)}")
        ps = self.param_groups[0]["params"]
        for p in ps:
            if not isinstance(p, torch.Tensor):
                raise TypeError(f"ClipAdam: parameters must be tensors, got {type(p).__name__}")
            if p.dtype != torch.float32:
                raise TypeError(f"ClipAdam: float32 parameters only, got {p.dtype}")
            if not p.is_cuda:
                raise ValueError("ClipAdam: parameters must be on a ROCm device (no CPU fallback)")
            if p.device != ps[0].device:
                raise ValueError(f"ClipAdam: parameters on one device, got {ps[0].device} and {p.device}")
            if not p.requires_grad:
                raise ValueError("ClipAdam: every parameter must require a gradient")
        self._params = list(ps)
        self._device = ps[0].device
        self._lib = _capi.load()
        self._views = FlatViews([tuple(p.shape) for p in ps])
        n = self._views.total
        plan = (ctypes.c_int64 * 3)()
        _capi.check(self._lib.wekws_hip_optim_plan(n, plan), "wekws_hip_optim_plan")
        assert self._lib.wekws_hip_optim_state_bytes() == _STATE_BYTES
        self._flat = torch.zeros(4, n, dtype=torch.float32, device=self._device)       # params, grads, exp_avg, exp_avg_sq
        self._state = torch.zeros(_STATE_BYTES, dtype=torch.uint8, device=self._device)
        self._workspace = torch.empty(int(plan[2]), dtype=torch.uint8, device=self._device)
        self._views.adopt(self._params, self._flat[0], self._flat[1])
        self._exp_avg = self._views.views(self._flat[2])
        self._exp_avg_sq = self._views.views(self._flat[3])

    def add_param_group(self, param_group) -> None:
        if self.param_groups:
            raise ValueError("ClipAdam: exactly one parameter group (the flat buffers are laid out at construction)")
        super().add_param_group(param_group)

    @staticmethod
    def _check_hyper(lr, betas, eps, weight_decay):
        if not 0.0 <= lr < math.inf:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps < math.inf:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if len(betas) != 2 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay < math.inf:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")

    # ------------------------------------------------------------------ the flat buffers and the state block
    @property
    def flat_params(self) -> torch.Tensor:
        return self._flat[0]

    @property
    def flat_grads(self) -> torch.Tensor:
        return self._flat[1]

    @property
    def steps(self) -> torch.Tensor:
        """() int64 on the device: steps applied so far."""
        return self._state.view(torch.int64)[_I64_STEP]

    @property
    def skipped_steps(self) -> torch.Tensor:
        """() int64 on the device: steps not applied because the gradient's norm was not finite."""
        return self._state.view(torch.int64)[_I64_SKIPPED]

    @property
    def last_clip_coef(self) -> torch.Tensor:
        """() float32 on the device: the coefficient the last step scaled the gradient by (1 without clipping)."""
        return self._state.view(torch.float32)[_F32_COEF]

    # ------------------------------------------------------------------ the step
    def zero_grad(self, set_to_none: bool = True) -> None:
        """One in-place ``zero_()`` of the flat gradient, whatever ``set_to_none`` says: a gradient set to None would leave the
        flat buffer (autograd would allocate a new one at the next backward), so the views are kept and zeroed."""
        self._flat[1].zero_()

    def _launch(self, max_norm: float, skip_nonfinite: int) -> None:
        bad = self._views.broken(self._params, self._flat[0], self._flat[1])
        if bad:
            raise RuntimeError("ClipAdam: the parameters no longer live in the optimiser's flat buffers (model.to(...), "
                               "p.grad = None or a zero_grad(set_to_none=True) from outside break the views; build the optimiser "
                               "after moving the model and use its own zero_grad): " + "; ".join(bad[:3]))
        g = self.param_groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("ClipAdam: amsgrad and maximize are not supported")
        lr, (beta1, beta2) = g["lr"], g["betas"]
        f = self._flat
        with torch.cuda.device(self._device):
            stream = ctypes.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)
            _capi.check(self._lib.wekws_hip_clip_adam_step(
                f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(), f[3].data_ptr(), self._views.total, self._state.data_ptr(),
                float(lr), float(beta1), float(beta2), float(g["eps"]), float(g["weight_decay"]), float(max_norm), skip_nonfinite,
                self._workspace.data_ptr(), self._workspace.numel(), stream), "wekws_hip_clip_adam_step")

    def clip_and_step(self, max_norm: float) -> torch.Tensor:
        """``grad_norm = clip_grad_norm_(params, max_norm); if isfinite(grad_norm): step()`` on the device.  Returns the norm of
        the unclipped gradient as a 0-dim float32 device tensor (a copy: it keeps its value over later steps); reads nothing."""
        self._launch(max_norm, 1)
        self._opt_called = True                         # what the wrapped step() sets: the schedulers' call-order warning reads it
        return self._state.view(torch.float32)[_F32_NORM].clone()

    @torch.no_grad()
    def step(self, closure=None):
        """Plain ``Adam.step()``: no clipping, applied whatever the gradient holds."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._launch(math.inf, 0)
        return loss

    # ------------------------------------------------------------------ torch.optim.Adam's state format
    def state_dict(self) -> dict:
        step = int(self.steps.item())                   # (a checkpoint reads the device anyway)
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self._params)))
        state = {}
        if step > 0:                                    # Adam has no state before its first step
            for i, (m, v) in enumerate(zip(self._exp_avg, self._exp_avg_sq)):
                state[i] = {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        return {"state": state, "param_groups": [group]}

    @torch.no_grad()
    def load_state_dict(self, state_dict: dict) -> None:
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._params):
            raise ValueError("ClipAdam: the state dict must hold one parameter group with as many parameters as the optimiser")
        new = groups[0]
        if new.get("amsgrad") or new.get("maximize"):
            raise ValueError("ClipAdam: amsgrad and maximize are not supported")
        self._check_hyper(new["lr"], new["betas"], new["eps"], new["weight_decay"])
        state = state_dict["state"]
        ids = list(new["params"])
        steps = set()
        if state:
            for i, pid in enumerate(ids):
                if pid not in state:
                    raise ValueError(f"ClipAdam: the state dict has no state for parameter {i} (one step counter serves all)")
                s = state[pid]
                steps.add(float(s["step"]))
                for key in ("exp_avg", "exp_avg_sq"):
                    if tuple(s[key].shape) != self._views.shapes[i]:
                        raise ValueError(f"ClipAdam: {key} of parameter {i} has shape {tuple(s[key].shape)}, expected {self._views.shapes[i]}")
            if len(steps) != 1:
                raise ValueError(f"ClipAdam: per-parameter steps differ ({sorted(steps)}); the optimiser keeps one global step")
        step = steps.pop() if steps else 0.0
        if step != int(step) or step < 0:
            raise ValueError(f"ClipAdam: step {step} is not a whole number")
        self._flat[2:].zero_()
        for i, pid in enumerate(ids if state else ()):
            self._exp_avg[i].copy_(state[pid]["exp_avg"])
            self._exp_avg_sq[i].copy_(state[pid]["exp_avg_sq"])
        self.steps.copy_(torch.tensor(int(step), dtype=torch.int64))
        for k in ("lr", "betas", "eps", "weight_decay"):
            self.param_groups[0][k] = tuple(new[k]) if k == "betas" else new[k]


def grad_norm(flat_grads: torch.Tensor) -> torch.Tensor:
    """The 2-norm of a flat float32 device tensor, summed in double in a fixed order (``wekws_hip_grad_norm``): a 0-dim
    float32 device tensor with the bits ``ClipAdam.clip_and_step`` returns for the same gradient."""
    if not isinstance(flat_grads, torch.Tensor) or not flat_grads.is_cuda or flat_grads.dtype != torch.float32 or flat_grads.dim() != 1 \
            or not flat_grads.is_contiguous() or flat_grads.numel() < 1:
        raise ValueError("grad_norm: a non-empty contiguous 1-dim float32 tensor on a ROCm device (no CPU fallback)")
    lib = _capi.load()
    plan = (ctypes.c_int64 * 3)()
    _capi.check(lib.wekws_hip_optim_plan(flat_grads.numel(), plan), "wekws_hip_optim_plan")
    dev = flat_grads.device
    ws = torch.empty(int(plan[2]), dtype=torch.uint8, device=dev)
    out = torch.empty((), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _capi.check(lib.wekws_hip_grad_norm(flat_grads.data_ptr(), flat_grads.numel(), out.data_ptr(), ws.data_ptr(), ws.numel(), stream),
                    "wekws_hip_grad_norm")
    return out
