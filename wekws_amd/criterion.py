"""The criterion on the device: wekws/model/loss.py::criterion (``max_pooling``, ``ce``, ``ctc``) -- what Executor.cv /
Executor.test call after every forward -- through ``wekws_hip_criterion_*`` / ``wekws_hip_ctc_loss`` /
``wekws_hip_ctc_edit_distance`` (csrc/criterion.hip.h), and its backward pass through ``wekws_hip_criterion_*_grad`` /
``wekws_hip_ctc_loss_grad`` (csrc/criterion_grad.hip.h).

When ``logits.requires_grad and torch.is_grad_enabled()`` the returned loss carries a ``grad_fn``: the forward is the very same
call (the same buffers, the same bits), and ``backward`` runs the gradient kernel with autograd's ``grad_output`` as a device
pointer and B as the divisor, so ``criterion(...)[0].backward()`` works for any torch module that produced ``logits`` on the
device.  ``ce`` and ``ctc`` differentiate with respect to the logits, ``max_pooling`` with respect to the posteriors it is
given; the accuracy outputs carry no gradient.  ``*_grad_device`` return the raw gradient tensors.

``criterion(type, logits, target, lengths, target_lengths=None, min_duration=0, validation=False)`` has the reference's
signature and returns ``(loss, acc)``: loss a 0-dim float32 device tensor, acc a Python float (reading it synchronises, as
the reference's ``.item()`` does).  ``criterion_device`` and the ``*_device`` functions return both as device tensors plus
the per-row outputs and never synchronise (the first ``ctc`` call with ``validation=True`` for a vocabulary creates the
decoder and its workspace, which does, once).

Deviations: frames beyond ``lengths`` are masked where the reference fails unless ``lengths.max() == T``;
a ``ce`` target outside [0, D) and a CTC label outside [1, V) make that row's loss NaN and the row incorrect where torch
raises; an unknown ``type`` raises ValueError where the reference calls ``exit(1)``."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import torch

from wekws_amd import _capi, _device

_Function = torch.autograd.Function


class MaxPoolingResult(NamedTuple):
    loss: torch.Tensor          # () float32
    acc: torch.Tensor           # () float64: num_correct / B
    pooled: torch.Tensor        # (B, K) float32
    loss_terms: torch.Tensor    # (B, K) float32
    correct: torch.Tensor       # (B) int32
    num_correct: torch.Tensor   # () int32


class CrossEntropyResult(NamedTuple):
    loss: torch.Tensor          # () float32
    acc: torch.Tensor           # () float64: num_correct * 100 / B
    loss_rows: torch.Tensor     # (B) float32
    pred: torch.Tensor          # (B) int32
    correct: torch.Tensor       # (B) int32
    num_correct: torch.Tensor   # () int32


class CtcResult(NamedTuple):
    loss: torch.Tensor                  # () float32
    acc: torch.Tensor                   # () float64; 0 without need_acc; NaN where the reference divides by zero
    loss_rows: torch.Tensor             # (B) float32
    distances: Optional[torch.Tensor]   # (B) int32 Levenshtein distance of the best hypothesis (need_acc)
    totals: Optional[torch.Tensor]      # (2) int32: label count, distance sum, over the rows with labels (need_acc)


def _f32(x: torch.Tensor, dim: int, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != dim:
        shape = "(B, T, K)" if dim == 3 else "(B, D)"
        raise ValueError(f"{what}: logits must be a {shape} float32 tensor on a ROCm device (no CPU fallback)")
    if 0 in x.shape:
        raise ValueError(f"{what}: empty logits {tuple(x.shape)}")
    return x.contiguous()


def _i32(v, n: int, dev: torch.device, what: str) -> torch.Tensor:
    if not isinstance(v, torch.Tensor) or not v.is_cuda:
        raise ValueError(f"{what} must be a tensor on a ROCm device (no CPU fallback)")
    t = v.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if t.numel() != n:
        raise ValueError(f"{what} must have {n} entries, got {t.numel()}")
    return t


def _scalar(v: int, dev: torch.device) -> torch.Tensor:
    """A float64 device scalar to divide by: tensor / tensor is a true division, whereas tensor / Python number is evaluated on
    the device as a product with the reciprocal (200 / 300 would come out one ulp above Python's)."""
    return torch.full((), float(v), dtype=torch.float64, device=dev)


def _wants_grad(logits) -> bool:
    return isinstance(logits, torch.Tensor) and logits.requires_grad and torch.is_grad_enabled()


def _upstream(upstream, dev: torch.device) -> Optional[torch.Tensor]:
    """None (the library reads 1), or one float32 on the device: a tensor is passed on by pointer, never read here."""
    if upstream is None:
        return None
    if isinstance(upstream, torch.Tensor):
        if not upstream.is_cuda or upstream.numel() != 1:
            raise ValueError("upstream must be one float on a ROCm device (no CPU fallback)")
        return upstream.to(device=dev, dtype=torch.float32).contiguous()
    return torch.full((), float(upstream), dtype=torch.float32, device=dev)


def _divisor(divisor, B: int) -> int:
    d = B if divisor is None else int(divisor)
    if d < 1:
        raise ValueError(f"divisor must be >= 1, got {d}")
    return d


def max_pooling_grad_device(logits: torch.Tensor, target: torch.Tensor, lengths: Optional[torch.Tensor], min_duration: int = 0,
                            upstream=None, divisor: Optional[int] = None) -> torch.Tensor:
    """d(max_pooling_loss) / d(logits) * upstream / divisor, (B, T, K) float32; ``divisor`` None: B (the batch loss)."""
    x = _f32(logits.detach(), 3, "max_pooling_grad")
    B, T, K = (int(v) for v in x.shape)
    dev = x.device
    tg = _i32(target, B, dev, "target")
    ln = None if lengths is None else _i32(lengths, B, dev, "lengths")
    up = _upstream(upstream, dev)
    grad = torch.empty((B, T, K), dtype=torch.float32, device=dev)
    _capi.check(_capi.load().wekws_hip_criterion_max_pooling_grad(
        x.data_ptr(), B, T, K, tg.data_ptr(), ln.data_ptr() if ln is not None else None, int(min_duration),
        up.data_ptr() if up is not None else None, _divisor(divisor, B), grad.data_ptr(), _device.stream(dev)),
        "wekws_hip_criterion_max_pooling_grad")
    return grad


def cross_entropy_grad_device(logits: torch.Tensor, target: torch.Tensor, upstream=None,
                              divisor: Optional[int] = None) -> torch.Tensor:
    """d(cross_entropy) / d(logits) * upstream / divisor, (B, D) float32."""
    x = _f32(logits.detach(), 2, "cross_entropy_grad")
    B, D = (int(v) for v in x.shape)
    dev = x.device
    tg = _i32(target, B, dev, "target")
    up = _upstream(upstream, dev)
    grad = torch.empty((B, D), dtype=torch.float32, device=dev)
    _capi.check(_capi.load().wekws_hip_criterion_ce_grad(x.data_ptr(), B, D, tg.data_ptr(), up.data_ptr() if up is not None else None,
                                                         _divisor(divisor, B), grad.data_ptr(), _device.stream(dev)),
                "wekws_hip_criterion_ce_grad")
    return grad


def ctc_loss_grad_device(logits: torch.Tensor, target: torch.Tensor, logits_lengths: torch.Tensor, target_lengths: torch.Tensor,
                         upstream=None, divisor: Optional[int] = None):
    """-> (grad (B, T, V), loss_rows (B), loss ()): d(ctc_loss) / d(logits) * upstream / divisor, and the loss with the bits
    of ``ctc_loss_device``."""
    x = _f32(logits.detach(), 3, "ctc_loss_grad")
    B, T, V = (int(v) for v in x.shape)
    dev = x.device
    if not isinstance(target, torch.Tensor) or not target.is_cuda:
        raise ValueError("target must be a tensor on a ROCm device (no CPU fallback)")
    tg = target.to(device=dev, dtype=torch.int32).reshape(B, -1).contiguous()
    Lmax = int(tg.size(1))
    ll = _i32(logits_lengths, B, dev, "logits_lengths")
    tl = _i32(target_lengths, B, dev, "target_lengths")
    up = _upstream(upstream, dev)
    lib = _capi.load()
    rows = torch.empty((B,), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    grad = torch.empty((B, T, V), dtype=torch.float32, device=dev)
    nbytes = int(lib.wekws_hip_ctc_loss_grad_workspace_bytes(B, T, Lmax))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    _capi.check(lib.wekws_hip_ctc_loss_grad(x.data_ptr(), B, T, V, tg.data_ptr() if Lmax else None, Lmax, ll.data_ptr(), tl.data_ptr(),
                                            up.data_ptr() if up is not None else None, _divisor(divisor, B), rows.data_ptr(),
                                            loss.data_ptr(), grad.data_ptr(), ws.data_ptr(), nbytes, _device.stream(dev)),
                "wekws_hip_ctc_loss_grad")
    return grad, rows, loss


class _MaxPoolingLoss(_Function):
    """loss = max_pooling_loss(logits): the forward call unchanged; backward: the gradient kernel, grad_output by pointer."""

    @staticmethod
    def forward(ctx, logits, target, lengths, min_duration, box):
        r = _max_pooling_forward(logits, target, lengths, min_duration)
        ctx.save_for_backward(logits, target, *([] if lengths is None else [lengths]))
        ctx.min_duration = min_duration
        box.append(r)
        return r.loss

    @staticmethod
    def backward(ctx, grad_output):
        logits, target, *rest = ctx.saved_tensors
        g = max_pooling_grad_device(logits, target, rest[0] if rest else None, ctx.min_duration, upstream=grad_output)
        return g, None, None, None, None


class _CrossEntropyLoss(_Function):

    @staticmethod
    def forward(ctx, logits, target, box):
        r = _cross_entropy_forward(logits, target)
        ctx.save_for_backward(logits, target)
        box.append(r)
        return r.loss

    @staticmethod
    def backward(ctx, grad_output):
        logits, target = ctx.saved_tensors
        return cross_entropy_grad_device(logits, target, upstream=grad_output), None, None


class _CtcLoss(_Function):

    @staticmethod
    def forward(ctx, logits, target, logits_lengths, target_lengths, need_acc, box):
        r = _ctc_loss_forward(logits, target, logits_lengths, target_lengths, need_acc)
        ctx.save_for_backward(logits, target, logits_lengths, target_lengths)
        box.append(r)
        return r.loss

    @staticmethod
    def backward(ctx, grad_output):
        logits, target, logits_lengths, target_lengths = ctx.saved_tensors
        g = ctc_loss_grad_device(logits, target, logits_lengths, target_lengths, upstream=grad_output)[0]
        return g, None, None, None, None, None


def max_pooling_loss_device(logits: torch.Tensor, target: torch.Tensor, lengths: Optional[torch.Tensor],
                            min_duration: int = 0) -> MaxPoolingResult:
    if not _wants_grad(logits):
        return _max_pooling_forward(logits, target, lengths, min_duration)
    box = []
    loss = _MaxPoolingLoss.apply(logits, target, lengths, int(min_duration), box)
    return box[0]._replace(loss=loss)


def cross_entropy_device(logits: torch.Tensor, target: torch.Tensor) -> CrossEntropyResult:
    if not _wants_grad(logits):
        return _cross_entropy_forward(logits, target)
    box = []
    loss = _CrossEntropyLoss.apply(logits, target, box)
    return box[0]._replace(loss=loss)


def ctc_loss_device(logits: torch.Tensor, target: torch.Tensor, logits_lengths: torch.Tensor,
                    target_lengths: torch.Tensor, need_acc: bool = False) -> CtcResult:
    if not _wants_grad(logits):
        return _ctc_loss_forward(logits, target, logits_lengths, target_lengths, need_acc)
    box = []
    loss = _CtcLoss.apply(logits, target, logits_lengths, target_lengths, bool(need_acc), box)
    return box[0]._replace(loss=loss)


def _max_pooling_forward(logits: torch.Tensor, target: torch.Tensor, lengths: Optional[torch.Tensor],
                         min_duration: int = 0) -> MaxPoolingResult:
    x = _f32(logits, 3, "max_pooling_loss")
    B, T, K = (int(v) for v in x.shape)
    dev = x.device
    tg = _i32(target, B, dev, "target")
    ln = None if lengths is None else _i32(lengths, B, dev, "lengths")
    pooled = torch.empty((B, K), dtype=torch.float32, device=dev)
    terms = torch.empty((B, K), dtype=torch.float32, device=dev)
    correct = torch.empty((B,), dtype=torch.int32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    num = torch.empty((), dtype=torch.int32, device=dev)
    _capi.check(_capi.load().wekws_hip_criterion_max_pooling(
        x.data_ptr(), B, T, K, tg.data_ptr(), ln.data_ptr() if ln is not None else None, int(min_duration), pooled.data_ptr(),
        terms.data_ptr(), correct.data_ptr(), loss.data_ptr(), num.data_ptr(), _device.stream(dev)), "wekws_hip_criterion_max_pooling")
    return MaxPoolingResult(loss, num.to(torch.float64) / _scalar(B, dev), pooled, terms, correct, num)


def _cross_entropy_forward(logits: torch.Tensor, target: torch.Tensor) -> CrossEntropyResult:
    x = _f32(logits, 2, "cross_entropy")
    B, D = (int(v) for v in x.shape)
    dev = x.device
    tg = _i32(target, B, dev, "target")
    rows = torch.empty((B,), dtype=torch.float32, device=dev)
    pred = torch.empty((B,), dtype=torch.int32, device=dev)
    correct = torch.empty((B,), dtype=torch.int32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    num = torch.empty((), dtype=torch.int32, device=dev)
    _capi.check(_capi.load().wekws_hip_criterion_ce(x.data_ptr(), B, D, tg.data_ptr(), rows.data_ptr(), pred.data_ptr(),
                                                    correct.data_ptr(), loss.data_ptr(), num.data_ptr(), _device.stream(dev)),
                "wekws_hip_criterion_ce")
    return CrossEntropyResult(loss, num.to(torch.float64) * 100.0 / _scalar(B, dev), rows, pred, correct, num)


_SCORE_BEAM, _PATH_BEAM = 3, 5            # acc_utterance: ctc_prefix_beam_search(score, length, None, 3, 5)
_decoders: Dict[Tuple[int, int], object] = {}


def _decoder(dev: torch.device, vocab: int):
    from wekws_amd.ctc import _Handle
    key = (dev.index or 0, vocab)
    if key not in _decoders:
        _decoders[key] = _Handle(key[0], vocab, [], None, _SCORE_BEAM, _PATH_BEAM)
    return _decoders[key]


def _ctc_loss_forward(logits: torch.Tensor, target: torch.Tensor, logits_lengths: torch.Tensor,
                      target_lengths: torch.Tensor, need_acc: bool = False) -> CtcResult:
    x = _f32(logits, 3, "ctc_loss")
    B, T, V = (int(v) for v in x.shape)
    dev = x.device
    if not isinstance(target, torch.Tensor) or not target.is_cuda:
        raise ValueError("target must be a tensor on a ROCm device (no CPU fallback)")
    tg = target.to(device=dev, dtype=torch.int32).reshape(B, -1).contiguous()
    Lmax = int(tg.size(1))
    ll = _i32(logits_lengths, B, dev, "logits_lengths")
    tl = _i32(target_lengths, B, dev, "target_lengths")
    lib = _capi.load()
    rows = torch.empty((B,), dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    nbytes = int(lib.wekws_hip_ctc_loss_workspace_bytes(B, T, Lmax))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    probs = torch.empty_like(x) if need_acc else None           # the posteriors of the decode, from the same read of the logits
    _capi.check(lib.wekws_hip_ctc_loss(x.data_ptr(), B, T, V, tg.data_ptr() if Lmax else None, Lmax, ll.data_ptr(), tl.data_ptr(),
                                       rows.data_ptr(), loss.data_ptr(), probs.data_ptr() if need_acc else None, ws.data_ptr(),
                                       nbytes, _device.stream(dev)), "wekws_hip_ctc_loss")
    if not need_acc:
        return CtcResult(loss, torch.zeros((), dtype=torch.float64, device=dev), rows, None, None)
    dist, totals = _utterance_distances(probs, tg, ll, tl)
    words = totals[0].to(torch.float64)
    acc = (totals[0] - totals[1]).to(torch.float64) * 100.0 / words       # 0 / 0 = NaN: the reference's ZeroDivisionError
    return CtcResult(loss, acc, rows, dist, totals)


def _utterance_distances(probs: torch.Tensor, tg: torch.Tensor, ll: torch.Tensor, tl: torch.Tensor):
    """acc_utterance after its softmax: the prefix beam search (no token set, beams 3 / 5) and the edit distance of its
    first hypothesis, on the device."""
    B, T, V = (int(v) for v in probs.shape)
    dev = probs.device
    lib = _capi.load()
    hd = _decoder(dev, V)
    res = torch.empty((B, 32), dtype=torch.uint8, device=dev)
    beams = torch.empty((B, hd.beam_bytes(T)), dtype=torch.uint8, device=dev)
    beams[:, :8].zero_()                  # a row whose search fails keeps no record: count 0, the empty hypothesis
    _capi.check(lib.wekws_hip_ctc_kws_search(hd.h, probs.data_ptr(), B, T, ll.clamp(0, T).data_ptr(), res.data_ptr(),
                                             beams.data_ptr(), _device.stream(dev)), "wekws_hip_ctc_kws_search")
    dist = torch.empty((B,), dtype=torch.int32, device=dev)
    totals = torch.empty((2,), dtype=torch.int32, device=dev)
    Lmax = int(tg.size(1))
    _capi.check(lib.wekws_hip_ctc_edit_distance(beams.data_ptr(), _PATH_BEAM, T, B, tg.data_ptr() if Lmax else None, Lmax,
                                                tl.data_ptr(), dist.data_ptr(), totals.data_ptr(), _device.stream(dev)),
                "wekws_hip_ctc_edit_distance")
    return dist, totals


def criterion_device(type: str, logits: torch.Tensor, target: torch.Tensor, lengths: torch.Tensor,
                     target_lengths: Optional[torch.Tensor] = None, min_duration: int = 0, validation: bool = False):
    """``criterion`` without a synchronise: the kind's result tuple (``.loss`` and ``.acc`` are device tensors)."""
    if type == "ce":
        return cross_entropy_device(logits, target)
    if type == "max_pooling":
        return max_pooling_loss_device(logits, target, lengths, min_duration)
    if type == "ctc":
        return ctc_loss_device(logits, target, lengths, target_lengths, validation)
    raise ValueError(f"unknown criterion {type!r} (ce, max_pooling, ctc)")


def max_pooling_loss(logits, target, lengths, min_duration: int = 0):
    r = max_pooling_loss_device(logits, target, lengths, min_duration)
    return r.loss, int(r.num_correct.item()) / int(logits.size(0))


def cross_entropy(logits, target):
    r = cross_entropy_device(logits, target)
    return r.loss, int(r.num_correct.item()) * 100.0 / int(logits.size(0))


def ctc_loss(logits, target, logits_lengths, target_lengths, need_acc: bool = False):
    r = ctc_loss_device(logits, target, logits_lengths, target_lengths, need_acc)
    if not need_acc:
        return r.loss, 0.0
    words, errors = (int(v) for v in r.totals.tolist())
    return r.loss, float(words - errors) * 100.0 / words         # ZeroDivisionError without a label, like the reference


def criterion(type: str, logits: torch.Tensor, target: torch.Tensor, lengths: torch.Tensor,
              target_lengths: Optional[torch.Tensor] = None, min_duration: int = 0, validation: bool = False):
    if type == "ce":
        return cross_entropy(logits, target)
    if type == "max_pooling":
        return max_pooling_loss(logits, target, lengths, min_duration)
    if type == "ctc":
        return ctc_loss(logits, target, lengths, target_lengths, validation)
    raise ValueError(f"unknown criterion {type!r} (ce, max_pooling, ctc)")
