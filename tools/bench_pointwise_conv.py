#!/usr/bin/env python3
"""Measurement: the pointwise Conv1d on the device (wekws_amd.model.pointwise) beside ``nn.Conv1d(kernel_size=1)`` on the same
tensors, on the same device in the same process:

    op        forward plus backward (all three gradients) at the recipes' shapes (B, Ci, Co, T) -- ds_tcn (256, 64, 64, 100),
              mdtc (100, 32, 32, 200), mdtc_pre (100, 80, 32, 200), ds256 (256, 256, 256, 100)
    step      the whole DS-TCN (256, 100, 40) and mdtc_small (100, 200, 80) training steps of DESIGN.md 3.21's table with
              use_device_pointwise_convs against without; use_device_batchnorms is on in both and the depthwise convolutions are
              the device's in both

Timing (DESIGN.md 3.21's protocol): both paths are warmed up, 0.3 s of work runs first, then 30 rounds alternate a group of 10
back-to-back calls of the device path with a group of 10 of torch's, each group between two device events; median / p10 / p90.
With ``--traces DIR`` -- DIR/<shape>/..._kernel_stats.csv from separate ``rocprofv3 --kernel-trace --stats`` runs of
``--only op_<shape>``, no counters -- an op's line also carries the average time of every kernel of that run, torch's among
them.  The bounds a kernel time is set against are computed here from the shape: FLOPs / 157 TF (the exact-float32 matrix rate)
and bytes / 8 TB/s.  GPU only; one JSON line per measurement.

    python tools/bench_pointwise_conv.py > profiles/pointwise_conv.jsonl"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_depthwise_conv import Kws, emit  # noqa: E402
from tools.bench_linear_wgrad import HBM_PEAK, MFMA_F32_PEAK, kernel_times  # noqa: E402
from wekws_amd import _capi  # noqa: E402
from wekws_amd.model import batchnorm, mdtc, pointwise, tcn  # noqa: E402

SHAPES = {"ds_tcn": (256, 64, 64, 100), "mdtc": (100, 32, 32, 200), "mdtc_pre": (100, 80, 32, 200), "ds256": (256, 256, 256, 100)}


def plan(B, Ci, T, Co):
    out = (ctypes.c_int64 * 7)()
    _capi.check(_capi.load().wekws_hip_pointwise_conv1d_plan(B, Ci, T, Co, out), "wekws_hip_pointwise_conv1d_plan")
    return dict(chain=out[0], chains=out[1], slices=out[2], wgrad_workgroups=out[3], workspace_bytes=out[4],
                forward_workgroups=out[5], dx_workgroups=out[6])


def bounds(B, Ci, Co, T, p):
    """What each of the three products costs at the least: 2 B T Ci Co FLOPs at the float32 matrix rate, and its operands and
    results once (the weight gradient's double partials written and read back) at the HBM rate."""
    flops = 2 * B * T * Ci * Co
    nx, ny, nw = 4 * B * Ci * T, 4 * B * Co * T, 4 * Co * Ci
    nbytes = dict(forward=nx + nw + 4 * Co + ny, dx=ny + nw + nx, wgrad=nx + ny + nw + 4 * Co + 2 * p["slices"] * (Co * Ci + Co) * 8)
    out = dict(flops_each=flops, flops_bound_us=round(flops / MFMA_F32_PEAK * 1e6, 2))
    for k, v in nbytes.items():
        out[f"{k}_bytes"] = v
        out[f"{k}_bytes_bound_us"] = round(v / HBM_PEAK * 1e6, 2)
    return out


def op_step(conv, x, g):
    def run():
        x.grad = None
        conv.weight.grad = None
        conv.bias.grad = None
        conv(x).backward(g)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="a substring of the measurement's name")
    ap.add_argument("--traces", default=None, help="directory of the rocprofv3 runs (see the module docstring)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pointwise_conv.py measures on the GPU only"
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    t = lambda shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)  # noqa: E731

    for shape, (B, Ci, Co, T) in SHAPES.items():
        name = f"op_{shape}"
        if a.only not in name:
            continue
        torch.manual_seed(0)
        theirs = nn.Conv1d(Ci, Co, 1).to(dev)
        ours = pointwise.PointwiseConv1d.sharing(theirs)
        x, g = t((B, Ci, T)).requires_grad_(), t((B, Co, T))
        p = plan(B, Ci, T, Co)
        extra = dict(shape=[B, Ci, Co, T], **p, **bounds(B, Ci, Co, T, p))
        if a.traces:
            extra["kernels_us_calls"] = kernel_times(a.traces, shape)
        emit(name, op_step(ours, x, g), op_step(theirs, x, g), **extra)

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
        runs, swapped = {}, 0
        for kind in ("torch_pointwise", "device_pointwise"):
            torch.manual_seed(0)
            model = Kws(idim, hdim, 1, make()).to(dev)
            batchnorm.use_device_batchnorms(model)
            if kind == "device_pointwise":
                swapped = pointwise.use_device_pointwise_convs(model)
            opt = ClipAdam(model.parameters(), lr=1e-3, weight_decay=5e-5)
            ex = TrainExecutor()
            runs[kind] = (lambda m=model, o=opt, e=ex: e.train(m, o, [batch], dev, None, args))
        emit(name, runs["device_pointwise"], runs["torch_pointwise"], parameters=sum(p.numel() for p in model.parameters()),
             pointwise_convs=swapped)


if __name__ == "__main__":
    main()
