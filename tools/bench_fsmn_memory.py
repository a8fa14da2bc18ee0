#!/usr/bin/env python3
"""Measurement: the FSMN memory block on the device (wekws_amd.model.fsmn) beside torch's own statements for the same block on
the same device in the same process:

    block     one block's forward + backward at (256, 100, 128) and (1024, 300, 128), taps (10, 2, 1, 1)     (fsmn_ctc.yaml)
              torch: the reference's statements -- permute, F.pad, two slices, two grouped Conv2d, two adds -- and autograd
    step      the full fsmn_ctc.yaml training step (FSMN 400-140-4x(250,128)-140-2599, ctc criterion, ClipAdam) on a batch of
              256 x 100 frames through TrainExecutor, with torch blocks and with device blocks

Timing as tools/bench_configs.py::timeit (warm-up, 0.3 s of work first, median / p10 / p90 of 30 groups of 10 back-to-back
steps between two device events).  Each block line carries the algorithmic bytes of the device path, computed from the shapes:
2 x B T D x 4 forward; 3 x B T D x 4 plus the partials backward, beside what the three backward kernels move (g twice, the
partials written and read back).  With `--trace FILE` (the kernel
statistics CSV of a separate `rocprofv3 --kernel-trace --stats` run of `--only block256`, the first shape alone) it adds each kernel's own time and its
share of the HBM rate (8.0 TB/s peak, 6.29 TB/s measured for a float4 copy).  GPU only; one JSON line per measurement.

    python tools/bench_fsmn_memory.py > profiles/fsmn_memory.jsonl"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_configs import timeit  # noqa: E402
from wekws_amd.model import fsmn  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
GRAD_TILE = 128                                   # csrc/fsmn_memory_plan.h
CTC = (400, 140, 4, 250, 128, 10, 2, 1, 1, 140, 2599)


class TorchBlock(torch.nn.Module):
    """The block's parameters under torch's own ops on the device: what the reference runs."""

    def __init__(self, block):
        super().__init__()
        self.lorder, self.rorder, self.lstride, self.rstride = block.lorder, block.rorder, block.lstride, block.rstride
        self.conv_left, self.conv_right = block.conv_left, block.conv_right

    def forward(self, input):
        x, in_cache = input if isinstance(input, tuple) else (input, torch.zeros(0, 0, 0, 0))
        pad = (self.lorder - 1) * self.lstride + self.rorder * self.rstride
        return fsmn.FSMNBlock._forward_torch(self, x, in_cache, pad)


def torch_blocks(model):
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, fsmn.FSMNBlock):
                setattr(parent, name, TorchBlock(child))
    return model


def block_bytes(B, T, D, lorder, rorder):
    tensor = B * T * D * 4
    partials = B * ((T + GRAD_TILE - 1) // GRAD_TILE) * (lorder + rorder) * D * 8
    # the algorithm needs g, x and dx once each and the partials once; the two backward kernels each read g, and the fold
    # reads the partials back
    return dict(forward_bytes=2 * tensor, input_grad_bytes=2 * tensor, tap_grad_bytes=2 * tensor + partials, fold_bytes=partials,
                backward_algorithmic_bytes=3 * tensor + partials, backward_bytes=4 * tensor + 2 * partials, partials_bytes=partials)


def trace_us(path, kernel):
    """Average duration of `kernel` in a rocprofv3 kernel-stats CSV, in microseconds."""
    with open(path) as f:
        for row in csv.DictReader(f):
            if kernel in row.get("Name", ""):
                return float(row["AverageNs"]) / 1e3
    return None


def emit(name, ours, theirs, **extra):
    med, p10, p90 = timeit(ours)
    tmed, tp10, tp90 = timeit(theirs)
    print(json.dumps(dict(name=name, ms=round(med, 4), p10=round(p10, 4), p90=round(p90, 4), torch_ms=round(tmed, 4),
                          torch_p10=round(tp10, 4), torch_p90=round(tp90, 4), torch_over_ours=round(tmed / med, 2), **extra)), flush=True)


def block_step(block, x, g):
    def run():
        x.grad = None
        block.conv_left.weight.grad = None
        block.conv_right.weight.grad = None
        y, _ = block((x, torch.zeros(0, 0, 0, 0)))
        y.backward(g)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--trace", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of `--only block256`")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fsmn_memory.py measures on the GPU only"
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)

    if a.only in ("", "block", "block256"):
        for B, T, D in ((256, 100, 128), (1024, 300, 128))[:1 if a.only == "block256" else 2]:
            torch.manual_seed(0)
            ours = fsmn.FSMNBlock(D, D, 10, 2, 1, 1).to(dev)
            theirs = TorchBlock(ours)
            x = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32)).to(dev).requires_grad_()
            g = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32)).to(dev)
            extra = block_bytes(B, T, D, 10, 2)
            if a.trace and (B, T) == (256, 100):
                for key, kernel, nbytes in (("forward", "fsmn_memory_fir_kernel<4, false>", extra["forward_bytes"]),
                                            ("input_grad", "fsmn_memory_fir_kernel<4, true>", extra["input_grad_bytes"]),
                                            ("tap_grad", "fsmn_memory_tap_grad_kernel", extra["tap_grad_bytes"]),
                                            ("fold", "fsmn_memory_fold_kernel", extra["fold_bytes"])):
                    us = trace_us(a.trace, kernel)
                    if us:
                        extra.update({f"{key}_us": round(us, 2), f"{key}_TBps": round(nbytes / (us * 1e-6) / 1e12, 3),
                                      f"{key}_share_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 3)})
            emit(f"block_{B}x{T}x{D}_taps10_2", block_step(ours, x, g), block_step(theirs, x, g), **extra)

    if a.only in ("", "step"):
        from wekws_amd.optim import ClipAdam
        from wekws_amd.utils.executor import TrainExecutor
        B, T, Lmax = 256, 100, 6
        batch = dict(feats=torch.from_numpy(rng.standard_normal((B, T, 400)).astype(np.float32)).to(dev),
                     target=torch.from_numpy(rng.integers(1, 2599, (B, Lmax)).astype(np.int64)).to(dev),
                     feats_lengths=torch.from_numpy(rng.integers(60, T + 1, B).astype(np.int32)).to(dev),
                     target_lengths=torch.from_numpy(rng.integers(3, Lmax + 1, B).astype(np.int32)).to(dev))
        args = {"criterion": "ctc", "grad_clip": 5.0, "log_interval": 1 << 30}
        runs = {}
        for kind in ("torch", "device"):
            torch.manual_seed(0)
            model = fsmn.FSMN(*CTC)
            model = (torch_blocks(model) if kind == "torch" else model).to(dev)
            opt = ClipAdam(model.parameters(), lr=1e-3, weight_decay=1e-4)
            ex = TrainExecutor()
            runs[kind] = (lambda m=model, o=opt, e=ex: e.train(m, o, [batch], dev, None, args))
        emit(f"train_step_fsmn_ctc_{B}x{T}", runs["device"], runs["torch"], parameters=sum(p.numel() for p in fsmn.FSMN(*CTC).parameters()))


if __name__ == "__main__":
    main()
