#!/usr/bin/env python3
"""Measurement: loss + gradient of the criterion per training step on the device (wekws_amd.criterion with a grad_fn) beside
the same statements run by torch on the same device in the same process, at the recipes' shapes:

    max_pooling  B = 256, T = 98 and 300, K = 2, min_duration 0 and 50     (ds_tcn.yaml)
                 torch: the reference's (utterance, keyword) loop restated, with its target.cpu()
    ctc          B = 256, T = 100, V = 2599, 3 ... 6 labels per row          (fsmn_ctc.yaml / ds_tcn_ctc.yaml after frame skip 3)
                 torch: log_softmax + F.ctc_loss(reduction='sum') / B
    ce           B = 100, D = 12                                              (speechcommand_v1)
                 torch: F.cross_entropy

Each side runs `loss(x); loss.backward()` on a leaf `x` that requires a gradient.  Timing as tools/bench_configs.py::timeit
(warm-up, 0.3 s of work first, median / p10 / p90 of 30 groups of 10 back-to-back steps between two device events).  For ctc
the line also carries the bytes the gradient path moves per step, computed from the shapes (below), and with `--trace FILE`
(the kernel statistics CSV of a separate `rocprofv3 --kernel-trace --stats` run of this tool) the gradient pass's own time
and its share of the HBM rate (8.0 TB/s peak, 6.29 TB/s measured for a float4 copy).  GPU only; one JSON line per measurement.

    python tools/bench_criterion_grad.py > profiles/criterion_grad.jsonl"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_configs import timeit  # noqa: E402
from wekws_amd import criterion as crit  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def torch_max_pooling(x, target, lengths, min_duration):
    """The reference's statements on the device: a Python loop over (utterance, keyword) after target.cpu()."""
    B, T, K = x.shape
    mask = torch.arange(T, device=x.device)[None, :] >= lengths[:, None]
    target = target.cpu()
    loss = 0.0
    for i in range(B):
        for j in range(K):
            if target[i] == j:
                m = mask[i].clone()
                m[:min_duration] = True
                loss = loss + -torch.log(torch.clamp(x[i, :, j].masked_fill(m, 0.0), 1e-8, 1.0).max())
            else:
                loss = loss + -torch.log(torch.clamp((1 - x[i, :, j]).masked_fill(mask[i], 1.0), 1e-8, 1.0).min())
    return loss / B


def torch_ctc(x, target, lengths, target_lengths):
    return F.ctc_loss(x.transpose(0, 1).log_softmax(2), target, lengths, target_lengths, reduction="sum") / x.size(0)


def step(loss_fn, x):
    def run():
        x.grad = None
        loss_fn(x).backward()
    return run


def ctc_bytes(B, T, V, Lmax, valid):
    """Bytes per training step of the ctc criterion: autograd's forward (wekws_hip_ctc_loss) and backward
    (wekws_hip_ctc_loss_grad); `valid`: the frames inside the rows' lengths -- the only ones whose logits are read."""
    W, frames = 2 * Lmax + 1, B * T
    logits, grad = valid * V * 4, frames * V * 4
    lp = valid * (Lmax + 1) * 4
    forward = logits + 2 * lp                                   # the log-sum pass reads the logits; lp written, read by alpha
    gradient_pass = logits + grad + valid * (W * 8 + 8)         # logits read, gradient written (zeros beyond the length), occupancies read
    backward = (logits + 2 * lp + valid * 8                     # the same pass again, with the frame statistics
                + lp + 3 * valid * W * 8                        # double alphas written, read and overwritten by the log-occupancies
                + gradient_pass)
    return dict(valid_frames=valid, frames=frames, logits_bytes_per_read=logits, forward_bytes=forward, backward_bytes=backward,
                gradient_pass_bytes=gradient_pass, logits_reads_per_step=3, gradient_writes_per_step=1)


def trace_time_us(path, kernel):
    """Average duration of `kernel` in a rocprofv3 kernel-stats CSV, in microseconds."""
    with open(path) as f:
        for row in csv.DictReader(f):
            if kernel in row.get("Name", ""):
                return float(row["AverageNs"]) / 1e3
    return None


def emit(name, ours, theirs, **extra):
    med, p10, p90 = timeit(ours)
    tmed, tp10, tp90 = timeit(theirs, warm=2, reps=extra.pop("torch_reps", 30), group=extra.pop("torch_group", 10))
    print(json.dumps(dict(name=name, ms=round(med, 4), p10=round(p10, 4), p90=round(p90, 4), torch_ms=round(tmed, 4),
                          torch_p10=round(tp10, 4), torch_p90=round(tp90, 4), torch_over_ours=round(tmed / med, 2), **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--trace", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of `--only ctc`")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_criterion_grad.py measures on the GPU only"
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)

    if a.only in ("", "max_pooling"):
        B, K = 256, 2
        for T, md in ((98, 0), (98, 50), (300, 50)):
            x = torch.from_numpy(rng.random((B, T, K), dtype=np.float32)).to(dev).requires_grad_()
            tg = torch.from_numpy(rng.integers(-1, K, B).astype(np.int32)).to(dev)
            ln = torch.from_numpy(rng.integers(T // 2, T + 1, B).astype(np.int32)).to(dev)
            ln[0] = T
            emit(f"max_pooling_{B}x{T}x{K}_md{md}", step(lambda v: crit.max_pooling_loss_device(v, tg, ln, md).loss, x),
                 step(lambda v: torch_max_pooling(v, tg, ln, md), x), torch_reps=5, torch_group=1)

    if a.only in ("", "ctc"):
        B, T, V, Lmax = 256, 100, 2599, 6
        x = torch.from_numpy((rng.standard_normal((B, T, V)) * 2).astype(np.float32)).to(dev).requires_grad_()
        tg = torch.from_numpy(rng.integers(1, V, (B, Lmax)).astype(np.int32)).to(dev)
        tl = torch.from_numpy(rng.integers(3, Lmax + 1, B).astype(np.int32)).to(dev)
        ln = torch.from_numpy(rng.integers(60, T + 1, B).astype(np.int32)).to(dev)
        tg64, tl64, ln64 = tg.long(), tl.long(), ln.long()
        extra = ctc_bytes(B, T, V, Lmax, int(ln.sum()))
        if a.trace:
            us = trace_time_us(a.trace, "ctc_grad_kernel")
            if us:
                rate = extra["gradient_pass_bytes"] / (us * 1e-6)
                extra.update(gradient_pass_us=round(us, 2), gradient_pass_TBps=round(rate / 1e12, 3),
                             gradient_pass_share_of_hbm_peak=round(rate / HBM_PEAK, 3),
                             gradient_pass_share_of_measured_copy=round(rate / HBM_COPY, 3))
        emit(f"ctc_{B}x{T}x{V}_labels3to{Lmax}", step(lambda v: crit.ctc_loss_device(v, tg, ln, tl).loss, x),
             step(lambda v: torch_ctc(v, tg64, ln64, tl64), x), **extra)

    if a.only in ("", "ce"):
        B, D = 100, 12
        x = torch.from_numpy((rng.standard_normal((B, D)) * 3).astype(np.float32)).to(dev).requires_grad_()
        tg = torch.from_numpy(rng.integers(0, D, B).astype(np.int32)).to(dev)
        tg64 = tg.long()
        emit(f"ce_{B}x{D}", step(lambda v: crit.cross_entropy_device(v, tg).loss, x), step(lambda v: F.cross_entropy(v, tg64), x))


if __name__ == "__main__":
    main()
