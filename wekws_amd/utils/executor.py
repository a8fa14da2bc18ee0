"""``Executor.cv`` / ``Executor.test`` of wekws/utils/executor.py:70-115 with the criterion on the device: the loop keeps
its running totals in float64 device scalars, so a whole evaluation moves two numbers to the host.  The totals follow the
reference statement by statement (``num_seen_utts`` starts at 1; a batch whose loss is not finite is skipped; ``loss.item()
* num_utts`` and ``acc * num_utts`` are float64 products added in batch order), so the result equals the host loop over the
same per-batch values bit for bit (tests/test_criterion_oracle.py).  ``Executor`` stays the evaluation loop of a packed,
inference-only KWSModel and its ``train`` raises; ``TrainExecutor.train`` is Executor.train of wekws/utils/executor.py:28-68
for a torch module on the device, with the criterion and its backward pass on the device (wekws_amd.criterion)."""
from __future__ import annotations

import logging

import torch
from torch.nn.utils import clip_grad_norm_

from wekws_amd.criterion import criterion_device


class RunningTotals:
    """The three accumulators of Executor.cv as tensors on ``device`` (CPU tensors work too: the arithmetic is torch's
    float64 either way)."""

    def __init__(self, device):
        self.num_seen_utts = torch.ones((), dtype=torch.int64, device=device)     # "in order to avoid division by 0"
        self.total_loss = torch.zeros((), dtype=torch.float64, device=device)
        self.total_acc = torch.zeros((), dtype=torch.float64, device=device)

    def add(self, loss: torch.Tensor, acc: torch.Tensor, num_utts: int) -> None:
        """``if torch.isfinite(loss): num_seen_utts += num_utts; total_loss += loss.item() * num_utts; total_acc += acc *
        num_utts`` without reading ``loss``.  A NaN ``acc`` (the accuracy the reference could not compute: its
        ZeroDivisionError) is kept whatever the loss, and surfaces in ``result``."""
        ok = torch.isfinite(loss)
        acc = acc.to(torch.float64)
        self.total_loss = torch.where(ok, self.total_loss + loss.to(torch.float64) * num_utts, self.total_loss)
        self.total_acc = torch.where(torch.isnan(acc), acc, torch.where(ok, self.total_acc + acc * num_utts, self.total_acc))
        self.num_seen_utts = torch.where(ok, self.num_seen_utts + num_utts, self.num_seen_utts)

    def result(self):
        """(total_loss / num_seen_utts, total_acc / num_seen_utts) as Python floats: the one read of the loop."""
        loss, acc = torch.stack([self.total_loss / self.num_seen_utts, self.total_acc / self.num_seen_utts]).tolist()
        if acc != acc:
            raise ZeroDivisionError("float division by zero")      # acc_utterance of a batch without a label (loss.py:131-132)
        return loss, acc


class Executor:

    def __init__(self):
        self.step = 0

    def train(self, model, optimizer, data_loader, device, writer, args):
        raise NotImplementedError("Executor runs packed, inference-only models: train a torch module with TrainExecutor")

    def cv(self, model, data_loader, device, args):
        model.eval()
        device = torch.device(device)
        totals = RunningTotals(device)
        kind = args.get('criterion', 'max_pooling')
        for batch_dict in data_loader:
            feats = batch_dict['feats']
            target = batch_dict['target']
            target = target[:, 0] if target.shape[1] == 1 else target
            feats_lengths = batch_dict['feats_lengths'].to(device)
            label_lengths = batch_dict['target_lengths'].to(device)
            num_utts = feats_lengths.size(0)
            if num_utts == 0:
                continue
            logits, _ = model(feats.to(device))
            r = criterion_device(kind, logits, target.to(device), feats_lengths, target_lengths=label_lengths, min_duration=0,
                                 validation=True)
            totals.add(r.loss, r.acc, num_utts)
        return totals.result()

    def test(self, model, data_loader, device, args):
        return self.cv(model, data_loader, device, args)


class TrainExecutor(Executor):
    """One epoch of training, statement by statement what the reference's Executor.train does -- ``min_duration`` and
    ``criterion`` from ``args``, zero_grad, backward, ``clip_grad_norm_(model.parameters(), args.get('grad_clip', 50.0))``, a
    step only when the norm is finite -- with ``criterion_device``: nothing but the log line every ``log_interval`` batches
    (formatted only when DEBUG logging is on) reads a value (``torch.isfinite(grad_norm)`` in the ``if`` is the reference's own read).  With an
    optimiser that has ``clip_and_step`` (wekws_amd.optim.ClipAdam) those three statements are that one call, on the device, and
    the step reads nothing on the host.  ``model`` is any torch module returning ``(logits, cache)``; differentiating it is
    torch's job."""

    def train(self, model, optimizer, data_loader, device, writer, args):
        model.train()
        clip = args.get('grad_clip', 50.0)
        log_interval = args.get('log_interval', 10)
        epoch = args.get('epoch', 0)
        min_duration = args.get('min_duration', 0)
        for batch_idx, batch_dict in enumerate(data_loader):
            target = batch_dict['target']
            target = target[:, 0] if target.shape[1] == 1 else target
            feats = batch_dict['feats'].to(device)
            target = target.to(device)
            feats_lengths = batch_dict['feats_lengths'].to(device)
            label_lengths = batch_dict['target_lengths'].to(device)
            num_utts = feats_lengths.size(0)
            if num_utts == 0:
                continue
            logits, _ = model(feats)
            r = criterion_device(args.get('criterion', 'max_pooling'), logits, target, feats_lengths,
                                 target_lengths=label_lengths, min_duration=min_duration, validation=False)
            optimizer.zero_grad()
            r.loss.backward()
            if hasattr(optimizer, 'clip_and_step'):
                grad_norm = optimizer.clip_and_step(clip)          # wekws_amd.optim.ClipAdam: the three statements on the device
            else:
                grad_norm = clip_grad_norm_(model.parameters(), clip)
                if torch.isfinite(grad_norm):
                    optimizer.step()
            if batch_idx % log_interval == 0 and logging.getLogger().isEnabledFor(logging.DEBUG):
                logging.debug('TRAIN Batch {}/{} loss {:.8f} acc {:.8f}'.format(epoch, batch_idx, r.loss.item(), float(r.acc)))
