#!/usr/bin/env python3
"""Measurement: the depthwise Conv1d on the device (wekws_amd.model.depthwise) beside torch's own statement for the same
convolution -- ``F.conv1d(F.pad(x, (P, 0)), w, b, dilation=d, groups=C)`` and its autograd -- on the same device in the same
process:

    conv      one convolution's forward + backward, full causal padding P = (K-1) d:
              (256, 64, 100) and (256, 256, 100) with K = 8, d in 1 and 8                      (ds_tcn.yaml blocks)
              (100, 32, 200) and (128, 64, 200) with K = 5, d in 1 and 8                       (mdtc_small.yaml / mdtc.yaml blocks)
    step      a whole training step through TrainExecutor (max_pooling criterion, ClipAdam), the depthwise convolutions swapped
              against unswapped: a DS-TCN backbone of 4 layers, 64 channels, kernel 8, batch 256 x 100 frames x 40, and the
              mdtc_small.yaml backbone (MDTC(3, 4, 32, 32, 5)), batch 100 x 200 frames x 80

Timing: both paths are warmed up, 0.3 s of work runs first, then 30 rounds alternate a group of 10 back-to-back steps of the
device path with a group of 10 of torch's, each group between two device events; median / p10 / p90 of the per-step time of a
path's 30 groups.  Each conv line carries the bytes the device kernels move, computed from the shapes.  With `--trace FILE`
(the kernel statistics CSV of a separate `rocprofv3 --kernel-trace --stats` run of `--only conv_256x64x100_k8_d8`) it adds each
kernel's own time and its share of the HBM rate (8.0 TB/s peak).  GPU only; one JSON line per measurement.

    python tools/bench_depthwise_conv.py > profiles/depthwise_conv.jsonl"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wekws_amd.model import depthwise, mdtc, tcn  # noqa: E402

HBM_PEAK = 8.0e12
GRAD_TILE = 128                                   # csrc/depthwise_conv_plan.h
CONVS = [(256, 64, 100, 8, 1), (256, 64, 100, 8, 8), (256, 256, 100, 8, 1), (256, 256, 100, 8, 8),
         (100, 32, 200, 5, 1), (100, 32, 200, 5, 8), (128, 64, 200, 5, 1), (128, 64, 200, 5, 8)]


class TorchConv1d(nn.Conv1d):
    """The convolution's parameters under torch's own statement on the device: what the reference runs."""

    def __init__(self, conv):
        super().__init__(conv.in_channels, conv.out_channels, conv.kernel_size[0], dilation=conv.dilation[0], groups=conv.groups,
                         bias=conv.bias is not None)
        self.weight, self.bias = conv.weight, conv.bias

    def forward(self, x, left_pad=0):
        return super().forward(F.pad(x, (left_pad, 0), value=0.0))


def torch_convs(model):
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, depthwise.DepthwiseConv1d):
                setattr(parent, name, TorchConv1d(child))
    return model


class Kws(nn.Module):
    """A keyword model around a backbone: Linear + ReLU in front, a Linear classifier and a sigmoid behind."""

    def __init__(self, idim, hdim, odim, backbone):
        super().__init__()
        self.pre = nn.Sequential(nn.Linear(idim, hdim), nn.ReLU())
        self.backbone = backbone
        self.head = nn.Linear(hdim, odim)

    def forward(self, x, cache=None):
        y, cache = self.backbone(self.pre(x), cache)
        return torch.sigmoid(self.head(y)), cache


def conv_bytes(B, C, T, K):
    tensor = B * C * T * 4                                        # full padding: Tout = Tin
    partials = B * ((T + GRAD_TILE - 1) // GRAD_TILE) * C * (K + 1) * 8
    # the algorithm needs x, g and dx once each and the partials once; the two backward kernels each read g, and the fold reads
    # the partials back.  (One tile a row at T <= 128: no halo is read twice.)
    return dict(forward_bytes=2 * tensor, input_grad_bytes=2 * tensor, tap_grad_bytes=2 * tensor + partials, fold_bytes=partials,
                backward_algorithmic_bytes=3 * tensor + partials, backward_bytes=4 * tensor + 2 * partials, partials_bytes=partials)


def trace_us(path, kernel):
    """Average duration of `kernel` in a rocprofv3 kernel-stats CSV, in microseconds."""
    with open(path) as f:
        for row in csv.DictReader(f):
            if kernel in row.get("Name", ""):
                return float(row["AverageNs"]) / 1e3
    return None


def time_alternating(ours, theirs, warm=5, reps=30, group=10):
    """-> ((median, p10, p90) of ours, the same of theirs), ms a step; groups of the two paths alternate."""
    for fn in (ours, theirs):
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t_pre = time.perf_counter()       # an idle MI355X runs its first ~0.25 s of work at lower clocks: measure behind that
    while time.perf_counter() - t_pre < 0.3:
        for _ in range(group):
            ours()
            theirs()
        torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(reps):
        for which, fn in enumerate((ours, theirs)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(group):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts[which].append(a.elapsed_time(b) / group)
    return tuple((float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))) for t in ts)


def emit(name, ours, theirs, **extra):
    (med, p10, p90), (tmed, tp10, tp90) = time_alternating(ours, theirs)
    print(json.dumps(dict(name=name, ms=round(med, 4), p10=round(p10, 4), p90=round(p90, 4), torch_ms=round(tmed, 4),
                          torch_p10=round(tp10, 4), torch_p90=round(tp90, 4), torch_over_ours=round(tmed / med, 2), **extra)), flush=True)


def conv_step(conv, x, g, P):
    def run():
        x.grad = None
        conv.weight.grad = None
        conv.bias.grad = None
        conv(x, P).backward(g)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="a substring of the measurement's name")
    ap.add_argument("--trace", default=None,
                    help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of `--only conv_256x64x100_k8_d8`")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depthwise_conv.py measures on the GPU only"
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)

    for B, C, T, K, d in CONVS:
        name = f"conv_{B}x{C}x{T}_k{K}_d{d}"
        if a.only not in name:
            continue
        torch.manual_seed(0)
        ours = depthwise.DepthwiseConv1d(C, C, K, dilation=d, groups=C).to(dev)
        theirs = TorchConv1d(ours)
        x = torch.from_numpy(rng.standard_normal((B, C, T)).astype(np.float32)).to(dev).requires_grad_()
        g = torch.from_numpy(rng.standard_normal((B, C, T)).astype(np.float32)).to(dev)
        extra = conv_bytes(B, C, T, K)
        if a.trace and (B, C, T, K, d) == (256, 64, 100, 8, 8):
            for key, kernel, nbytes in (("forward", "depthwise_conv_fir_kernel<4, false>", extra["forward_bytes"]),
                                        ("input_grad", "depthwise_conv_fir_kernel<4, true>", extra["input_grad_bytes"]),
                                        ("tap_grad", "depthwise_conv_tap_grad_kernel", extra["tap_grad_bytes"]),
                                        ("fold", "depthwise_conv_fold_kernel", extra["fold_bytes"])):
                us = trace_us(a.trace, kernel)
                if us:
                    extra.update({f"{key}_us": round(us, 2), f"{key}_TBps": round(nbytes / (us * 1e-6) / 1e12, 3),
                                  f"{key}_share_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 3)})
        emit(name, conv_step(ours, x, g, (K - 1) * d), conv_step(theirs, x, g, (K - 1) * d), **extra)

    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    steps = (("train_step_ds_tcn_4x64_k8_256x100", 256, 100, 40, 64, lambda: tcn.TCN(4, 64, 8, block_class=tcn.DsCnnBlock)),
             ("train_step_mdtc_small_100x200", 100, 200, 80, 32, lambda: mdtc.MDTC(3, 4, 32, 32, 5, True)))
    for name, B, T, idim, hdim, make in steps:
        if a.only not in name:
            continue
        batch = dict(feats=torch.from_numpy(rng.standard_normal((B, T, idim)).astype(np.float32)).to(dev),
                     target=torch.from_numpy(rng.integers(-1, 1, (B, 1)).astype(np.int64)).to(dev),
                     feats_lengths=torch.from_numpy(rng.integers(T // 2, T + 1, B).astype(np.int32)).to(dev),
                     target_lengths=torch.ones(B, dtype=torch.int32, device=dev))
        args = {"criterion": "max_pooling", "grad_clip": 5.0, "log_interval": 1 << 30}
        runs = {}
        for kind in ("torch", "device"):
            torch.manual_seed(0)
            model = Kws(idim, hdim, 1, make())
            model = (torch_convs(model) if kind == "torch" else model).to(dev)
            opt = ClipAdam(model.parameters(), lr=1e-3, weight_decay=5e-5)
            ex = TrainExecutor()
            runs[kind] = (lambda m=model, o=opt, e=ex: e.train(m, o, [batch], dev, None, args))
            convs = sum(isinstance(m, depthwise.DepthwiseConv1d) for m in model.modules())
        emit(name, runs["device"], runs["torch"], parameters=sum(p.numel() for p in model.parameters()), depthwise_convs=convs)


if __name__ == "__main__":
    main()
