#!/usr/bin/env python3
"""Measurement: the fused BatchNorm1d on the device (wekws_amd.model.batchnorm) beside torch's own statements for the same site
-- ``F.relu(bn(x) + residual)`` and its autograd -- on the same device in the same process:

    site      one site's forward + backward in train(), the three kinds bn (DSDilatedConv1d.bn), bn_relu (DsCnnBlock.cnn[1:3],
              TCNBlock.bn1 / relu1) and bn_res_relu (TCNBlock.bn2 + inputs + relu2) at (256, 64, 100), (256, 256, 100),
              (100, 32, 200) and (128, 64, 200)
    step      a whole training step through TrainExecutor (max_pooling criterion, ClipAdam) with device depthwise convolutions
              in both runs, use_device_batchnorms against torch's BatchNorms: a DS-TCN backbone of 4 layers, 64 channels,
              kernel 8, batch 256 x 100 frames x 40, and the mdtc_small.yaml backbone (MDTC(3, 4, 32, 32, 5)), batch 100 x 200
              frames x 80

Timing: both paths are warmed up, 0.3 s of work runs first, then 30 rounds alternate a group of 10 back-to-back steps of the
device path with a group of 10 of torch's, each group between two device events; median / p10 / p90 of the per-step time of a
path's 30 groups.  Each site line carries the bytes the device kernels move, computed from the shapes.  With `--trace FILE`
(the kernel statistics CSV of a separate `rocprofv3 --kernel-trace --stats` run of `--only site_bn_res_relu_256x64x100`) it adds
each kernel's own time and its share of the HBM rate (8.0 TB/s peak).  GPU only; one JSON line per measurement.

    python tools/bench_batchnorm.py > profiles/batchnorm.jsonl"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_depthwise_conv import HBM_PEAK, Kws, emit, trace_us  # noqa: E402
from wekws_amd.model import batchnorm, mdtc, tcn  # noqa: E402

TILE = 128                                        # csrc/batchnorm_plan.h
SHAPES = [(256, 64, 100), (256, 256, 100), (100, 32, 200), (128, 64, 200)]
KINDS = {"bn": (False, False), "bn_relu": (True, False), "bn_res_relu": (True, True)}       # kind -> (relu, residual)


def site_bytes(B, C, T, relu, residual):
    tensor = B * C * T * 4
    partials = B * ((T + TILE - 1) // TILE) * C * 2 * 8
    stats, apply = tensor + partials, (2 + residual) * tensor
    sums = (2 + relu) * tensor + partials                         # x, g and, under a ReLU, y
    grad_x = (3 + relu + (residual and relu)) * tensor            # g, x, dx; y under a ReLU; grad_residual where it is not grad_y itself
    return dict(stats_bytes=stats, stats_fold_bytes=partials, apply_bytes=apply, grad_sums_bytes=sums, grad_fold_bytes=partials,
                grad_x_bytes=grad_x, total_bytes=stats + apply + sums + grad_x + 2 * partials)


def site_step(bn, x, res, g, relu, fused):
    def run():
        x.grad = None
        bn.weight.grad = None
        bn.bias.grad = None
        if res is not None:
            res.grad = None
        if fused:
            y = bn(x, residual=res, relu=relu)
        else:
            y = bn(x)
            y = y + res if res is not None else y
            y = F.relu(y) if relu else y
        y.backward(g)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="a substring of the measurement's name")
    ap.add_argument("--trace", default=None,
                    help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of `--only site_bn_res_relu_256x64x100`")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_batchnorm.py measures on the GPU only"
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    t = lambda shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)  # noqa: E731

    for B, C, T in SHAPES:
        for kind, (relu, residual) in KINDS.items():
            name = f"site_{kind}_{B}x{C}x{T}"
            if a.only not in name:
                continue
            ours = batchnorm.DeviceBatchNorm1d(C).to(dev)
            theirs = nn.BatchNorm1d(C).to(dev)
            x, g = t((B, C, T)).requires_grad_(), t((B, C, T))
            res = t((B, C, T)).requires_grad_() if residual else None
            extra = site_bytes(B, C, T, relu, residual)
            if a.trace and (kind, B, C, T) == ("bn_res_relu", 256, 64, 100):
                for key, kernel in (("stats", "batchnorm_stats_kernel"), ("stats_fold", "batchnorm_stats_fold_kernel"),
                                    ("apply", "batchnorm_apply_kernel"), ("grad_sums", "batchnorm_grad_sums_kernel"),
                                    ("grad_fold", "batchnorm_grad_fold_kernel"), ("grad_x", "batchnorm_grad_x_kernel")):
                    us = trace_us(a.trace, kernel)
                    if us:
                        nbytes = extra[f"{key}_bytes"]
                        extra.update({f"{key}_us": round(us, 2), f"{key}_TBps": round(nbytes / (us * 1e-6) / 1e12, 3),
                                      f"{key}_share_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 3)})
            emit(name, site_step(ours, x, res, g, relu, True), site_step(theirs, x, res, g, relu, False), **extra)

    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    steps = (("train_step_ds_tcn_4x64_k8_256x100", 256, 100, 40, 64, lambda: tcn.TCN(4, 64, 8, block_class=tcn.DsCnnBlock)),
             ("train_step_mdtc_small_100x200", 100, 200, 80, 32, lambda: mdtc.MDTC(3, 4, 32, 32, 5, True)))
    for name, B, T, idim, hdim, make in steps:
        if a.only not in name:
            continue
        batch = dict(feats=t((B, T, idim)), target=torch.from_numpy(rng.integers(-1, 1, (B, 1)).astype(np.int64)).to(dev),
                     feats_lengths=torch.from_numpy(rng.integers(T // 2, T + 1, B).astype(np.int32)).to(dev),
                     target_lengths=torch.ones(B, dtype=torch.int32, device=dev))
        args = {"criterion": "max_pooling", "grad_clip": 5.0, "log_interval": 1 << 30}
        torch.manual_seed(0)
        base = Kws(idim, hdim, 1, make())
        runs, norms = {}, 0
        for kind in ("torch", "device"):
            model = copy.deepcopy(base).to(dev)
            if kind == "device":
                norms = batchnorm.use_device_batchnorms(model)
            opt = ClipAdam(model.parameters(), lr=1e-3, weight_decay=5e-5)
            ex = TrainExecutor()
            runs[kind] = (lambda m=model, o=opt, e=ex: e.train(m, o, [batch], dev, None, args))
        emit(name, runs["device"], runs["torch"], parameters=sum(p.numel() for p in base.parameters()), batchnorms=norms)


if __name__ == "__main__":
    main()
