#!/usr/bin/env python3
"""Measurement: the trainable GRU on the device (wekws_amd.model.gru) beside torch's own ``nn.GRU`` over the same parameters, on
the same device in the same process:

    gru       forward + backward of the 2 x 128 GRU of examples/hi_xiaowen/s0/conf/gru.yaml at (256, 100, 128), the recipe's
              batch, and at (1024, 300, 128)
    step      the whole gru.yaml training step through TrainExecutor (max_pooling criterion, ClipAdam, grad_clip 5), batch
              256 x 100 frames x 40, with use_device_grus against torch's nn.GRU

Timing (DESIGN.md 3.21's protocol): both paths are warmed up, 0.3 s of work runs first, then 30 rounds alternate a group of 10
back-to-back steps of the device path with a group of 10 of torch's, each group between two device events; median / p10 / p90
of the per-step time of a path's 30 groups.  With `--trace FILE` (the kernel statistics CSV of a separate
`rocprofv3 --kernel-trace --stats` run of `--only gru_2x128_256x100`, no counters) it adds the two scan kernels' own times.  GPU
only; one JSON line per measurement.

    python tools/bench_gru_train.py > profiles/gru_train.jsonl"""
import argparse
import copy
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_depthwise_conv import Kws, emit, trace_us  # noqa: E402
from wekws_amd.model import gru as dg  # noqa: E402

SHAPES = [(256, 100, 128), (1024, 300, 128)]
LAYERS = 2


def gru_step(m, x, g):
    def run():
        x.grad = None
        for p in m.parameters():
            p.grad = None
        y, _ = m(x)
        y.backward(g)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="a substring of the measurement's name")
    ap.add_argument("--trace", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of `--only gru_2x128_256x100`")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gru_train.py measures on the GPU only"
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    t = lambda shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)  # noqa: E731

    for B, T, H in SHAPES:
        name = f"gru_{LAYERS}x{H}_{B}x{T}"
        if a.only not in name:
            continue
        torch.manual_seed(0)
        theirs = nn.GRU(H, H, num_layers=LAYERS, batch_first=True).to(dev)
        ours = dg.DeviceGRU.sharing(theirs)
        x, g = t((B, T, H)).requires_grad_(), t((B, T, H))
        # per layer and direction of time: 3 H/4 MFMAs of 16x16x4 per wave and step, H/16 waves, ceil(B/16) workgroups
        extra = dict(workgroups=(B + 15) // 16, scan_flops=2 * 2 * LAYERS * B * T * 3 * H * H)
        if a.trace and (B, T) == (256, 100):
            for key, kernel in (("scan_fwd", "gru_scan_fwd"), ("scan_bwd", "gru_scan_bwd")):
                us = trace_us(a.trace, kernel)
                if us:
                    extra[f"{key}_us"] = round(us, 2)
        emit(name, gru_step(ours, x, g), gru_step(theirs, x, g), **extra)

    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    name, B, T, idim, hdim = "train_step_gru_yaml_256x100", 256, 100, 40, 128
    if a.only in name:
        batch = dict(feats=t((B, T, idim)), target=torch.from_numpy(rng.integers(-1, 1, (B, 1)).astype(np.int64)).to(dev),
                     feats_lengths=torch.from_numpy(rng.integers(T // 2, T + 1, B).astype(np.int32)).to(dev),
                     target_lengths=torch.ones(B, dtype=torch.int32, device=dev))
        args = {"criterion": "max_pooling", "grad_clip": 5.0, "log_interval": 1 << 30}
        torch.manual_seed(0)
        base = Kws(idim, hdim, 1, nn.GRU(hdim, hdim, num_layers=LAYERS, batch_first=True))
        runs, swapped = {}, 0
        for kind in ("torch", "device"):
            model = copy.deepcopy(base).to(dev)
            if kind == "device":
                swapped = dg.use_device_grus(model)
            opt = ClipAdam(model.parameters(), lr=1e-3, weight_decay=5e-5)
            ex = TrainExecutor()
            runs[kind] = (lambda m=model, o=opt, e=ex: e.train(m, o, [batch], dev, None, args))
        emit(name, runs["device"], runs["torch"], parameters=sum(p.numel() for p in base.parameters()), grus=swapped)


if __name__ == "__main__":
    main()
