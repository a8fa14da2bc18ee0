#!/usr/bin/env python3
"""Measurement: the dense dilated Conv1d on the device (wekws_amd.model.dense) beside ``nn.Conv1d`` behind ``F.pad`` on the same
tensors, on the same device in the same process:

    op        forward plus backward (all three gradients) at the recipe's shapes (B, Ci, Co, Tin, K, d, left_pad) -- the four
              layers of tcn.yaml, (256, 64, 64, 100, 8, d, 7 d) for d = 1, 2, 4, 8 -- and the Conv1dSubsampling1 shape
              (256, 40, 64, 100, 3, 1, 0)
    step      the whole tcn.yaml training step, TCN(4, 64, 8, CnnBlock) at 256 x 100 frames x 40, with use_device_dense_convs
              against without; use_device_batchnorms, use_device_weight_grads and ClipAdam are on in both

Timing (DESIGN.md 3.21's protocol): both paths are warmed up, 0.3 s of work runs first, then 30 rounds alternate a group of 10
back-to-back calls of the device path with a group of 10 of torch's, each group between two device events; median / p10 / p90.
With ``--traces DIR`` -- DIR/<shape>/..._kernel_stats.csv from separate ``rocprofv3 --kernel-trace --stats`` runs of
``--only op_<shape>``, no counters -- an op's line also carries the average time of every kernel of that run, torch's among
them.  The bounds a kernel time is set against are computed here from the shape: FLOPs / 157 TF (the exact-float32 matrix rate)
and bytes / 8 TB/s.  GPU only; one JSON line per measurement.

    python tools/bench_dense_conv.py > profiles/dense_conv.jsonl"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_depthwise_conv import Kws, emit  # noqa: E402
from tools.bench_linear_wgrad import HBM_PEAK, MFMA_F32_PEAK, kernel_times  # noqa: E402
from wekws_amd import _capi  # noqa: E402
from wekws_amd.model import batchnorm, dense, linear, tcn  # noqa: E402

SHAPES = {f"tcn_d{d}": (256, 64, 64, 100, 8, d, 7 * d) for d in (1, 2, 4, 8)}
SHAPES["subsampling"] = (256, 40, 64, 100, 3, 1, 0)


def plan(B, Ci, Tin, Co, K, d, P):
    out = (ctypes.c_int64 * 10)()
    _capi.check(_capi.load().wekws_hip_dense_conv1d_plan(B, Ci, Tin, Co, K, d, P, out), "wekws_hip_dense_conv1d_plan")
    return dict(chain=out[0], chains=out[1], slices=out[2], wgrad_workgroups_a_tap=out[3], workspace_bytes=out[4],
                forward_workgroups=out[5], dx_workgroups=out[6], taps=out[7], fold_workgroups_a_tap=out[8], Tout=out[9])


def bounds(B, Ci, Co, Tin, K, p):
    """What each of the three products costs at the least: 2 B Tout K Ci Co FLOPs at the float32 matrix rate, and its operands
    and results once (the weight gradient's double partials written and read back) at the HBM rate."""
    Tout = p["Tout"]
    flops = 2 * B * Tout * K * Ci * Co
    nx, ny, nw = 4 * B * Ci * Tin, 4 * B * Co * Tout, 4 * Co * Ci * K
    nbytes = dict(forward=nx + nw + 4 * Co + ny, dx=ny + nw + nx, wgrad=nx + ny + nw + 4 * Co + 2 * p["slices"] * (K * Co * Ci + Co) * 8)
    out = dict(flops_each=flops, flops_bound_us=round(flops / MFMA_F32_PEAK * 1e6, 2))
    for k, v in nbytes.items():
        out[f"{k}_bytes"] = v
        out[f"{k}_bytes_bound_us"] = round(v / HBM_PEAK * 1e6, 2)
    return out


def op_step(conv, x, g, call):
    def run():
        x.grad = None
        conv.weight.grad = None
        conv.bias.grad = None
        call(x).backward(g)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="a substring of the measurement's name")
    ap.add_argument("--traces", default=None, help="directory of the rocprofv3 runs (see the module docstring)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dense_conv.py measures on the GPU only"
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    t = lambda shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)  # noqa: E731

    for shape, (B, Ci, Co, Tin, K, d, P) in SHAPES.items():
        name = f"op_{shape}"
        if a.only not in name:
            continue
        torch.manual_seed(0)
        theirs = nn.Conv1d(Ci, Co, K, dilation=d).to(dev)
        ours = dense.DenseConv1d.sharing(theirs)
        p = plan(B, Ci, Tin, Co, K, d, P)
        x, g = t((B, Ci, Tin)).requires_grad_(), t((B, Co, p["Tout"]))
        extra = dict(shape=[B, Ci, Co, Tin, K, d, P], **p, **bounds(B, Ci, Co, Tin, K, p))
        if a.traces:
            extra["kernels_us_calls"] = kernel_times(a.traces, shape)
        emit(name, op_step(ours, x, g, lambda v: ours(v, P)), op_step(theirs, x, g, lambda v: theirs(F.pad(v, (P, 0), value=0.0))), **extra)

    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    name, B, T, idim, hdim = "train_step_tcn_4x64_k8_256x100", 256, 100, 40, 64
    if a.only in name:
        batch = dict(feats=t((B, T, idim)), target=torch.from_numpy(rng.integers(-1, 1, (B, 1)).astype(np.int64)).to(dev),
                     feats_lengths=torch.from_numpy(rng.integers(T // 2, T + 1, B).astype(np.int32)).to(dev),
                     target_lengths=torch.ones(B, dtype=torch.int32, device=dev))
        args = {"criterion": "max_pooling", "grad_clip": 5.0, "log_interval": 1 << 30}
        runs, swapped = {}, 0
        for kind in ("torch_dense", "device_dense"):
            torch.manual_seed(0)
            model = Kws(idim, hdim, 1, tcn.TCN(4, 64, 8, block_class=tcn.CnnBlock)).to(dev)
            batchnorm.use_device_batchnorms(model)
            linear.use_device_weight_grads(model)
            if kind == "device_dense":
                swapped = dense.use_device_dense_convs(model)
            opt = ClipAdam(model.parameters(), lr=1e-3, weight_decay=5e-5)
            ex = TrainExecutor()
            runs[kind] = (lambda m=model, o=opt, e=ex: e.train(m, o, [batch], dev, None, args))
        emit(name, runs["device_dense"], runs["torch_dense"], parameters=sum(p.numel() for p in model.parameters()), dense_convs=swapped)


if __name__ == "__main__":
    main()
