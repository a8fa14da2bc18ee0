#!/usr/bin/env python3
"""Measurement: the Linear layers' weight and bias gradients on the device (wekws_amd.model.linear) beside torch's own
``g.t().mm(x)`` + ``g.sum(0)`` on the same tensors, on the same device in the same process:

    op        linear_weight_grad at the recipes' shapes (R, O, I) -- gru_ih (25600, 384, 128), fsmn_in (25600, 140, 400),
              fsmn_blk (25600, 128, 250), cls (4096, 2599, 140) -- and at (4096, 128, 128)
    step      the whole gru.yaml training step (DESIGN.md 3.23's set-up, device GRUs) and the whole fsmn_ctc.yaml step (3.20's,
              device memory blocks), each with use_device_weight_grads against without
    units     the error of the GRU's weight gradients at the ``recipe`` case of tests/gru_train_matrix.py, with the switch off
              and on, in that file's units

Timing (DESIGN.md 3.21's protocol): both paths are warmed up, 0.3 s of work runs first, then 30 rounds alternate a group of 10
back-to-back calls of the device path with a group of 10 of torch's, each group between two device events; median / p10 / p90.
With ``--traces DIR`` -- DIR/<shape>/..._kernel_stats.csv from separate ``rocprofv3 --kernel-trace --stats`` runs of
``--only op_<shape>``, no counters -- an op's line also carries the average time of every kernel of that run.  The bounds a kernel
time is set against are computed here from the shape: FLOPs / 157 TF (the exact-float32 matrix rate) and bytes / 8 TB/s.  GPU only;
one JSON line per measurement.

    python tools/bench_linear_wgrad.py > profiles/linear_wgrad.jsonl"""
import argparse
import copy
import csv
import ctypes
import glob
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_depthwise_conv import Kws, emit  # noqa: E402
from tools.bench_fsmn_memory import CTC  # noqa: E402
from wekws_amd import _capi  # noqa: E402
from wekws_amd.model import fsmn  # noqa: E402
from wekws_amd.model import gru as dg  # noqa: E402
from wekws_amd.model import linear as dl  # noqa: E402

SHAPES = {"gru_ih": (25600, 384, 128), "fsmn_in": (25600, 140, 400), "fsmn_blk": (25600, 128, 250), "cls": (4096, 2599, 140),
          "sq128": (4096, 128, 128)}
MFMA_F32_PEAK, HBM_PEAK = 157e12, 8e12


def plan(R, O, I):
    out = (ctypes.c_int64 * 5)()
    _capi.check(_capi.load().wekws_hip_linear_wgrad_plan(R, O, I, out), "wekws_hip_linear_wgrad_plan")
    return dict(chain=out[0], chains=out[1], slices=out[2], workgroups=out[3], workspace_bytes=out[4])


def bounds(R, O, I, p):
    """What the shape costs at the least: the product's FLOPs at the float32 matrix rate, and the bytes of x, g, dw and db once
    plus the double partials written and read back, at the HBM rate."""
    flops = 2 * R * O * I
    pad = lambda n: -(-n // 64) * 64  # noqa: E731
    partials = p["slices"] * (O * I + O) * 8
    nbytes = 4 * (R * I + R * O + O * I + O) + 2 * partials
    # what the partial kernel fetches: every tile re-reads its 64 columns of g and of x
    fetched = 4 * R * (pad(O) // 64) * (pad(I) // 64) * 128
    t_flops, t_bytes = flops / MFMA_F32_PEAK, nbytes / HBM_PEAK
    return dict(flops=flops, algorithmic_bytes=nbytes, fetched_bytes=fetched, flops_bound_us=round(t_flops * 1e6, 2),
                bytes_bound_us=round(t_bytes * 1e6, 2), bound="flops" if t_flops >= t_bytes else "bytes")


def kernel_times(traces, shape):
    """{kernel name (shortened): (average us, calls)} of the rocprofv3 run of one shape."""
    files = glob.glob(os.path.join(traces, shape, "**", "*kernel_stats.csv"), recursive=True)
    out = {}
    for path in files[:1]:
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                short = name.split("(")[0][:60]
                out[short] = (round(float(row["AverageNs"]) / 1e3, 2), int(row["Calls"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", help="a substring of the measurement's name")
    ap.add_argument("--traces", default=None, help="directory of the rocprofv3 runs (see the module docstring)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_linear_wgrad.py measures on the GPU only"
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    t = lambda shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)  # noqa: E731

    for shape, (R, O, I) in SHAPES.items():
        name = f"op_{shape}"
        if a.only not in name:
            continue
        x, g = t((R, I)), t((R, O))
        p = plan(R, O, I)
        extra = dict(shape=[R, O, I], **p, **bounds(R, O, I, p))
        if a.traces:
            extra["kernels_us_calls"] = kernel_times(a.traces, shape)
        emit(name, lambda: dl.linear_weight_grad(x, g), lambda: (g.t().mm(x), g.sum(0)), **extra)

    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor

    def step_pair(name, base, batch, args, prepare, **hyper):
        runs, changed = {}, 0
        for kind in ("torch_wgrads", "device_wgrads"):
            model = copy.deepcopy(base).to(dev)
            prepare(model)
            if kind == "device_wgrads":
                changed = dl.use_device_weight_grads(model)
            opt = ClipAdam(model.parameters(), **hyper)
            ex = TrainExecutor()
            runs[kind] = (lambda m=model, o=opt, e=ex: e.train(m, o, [batch], dev, None, args))
        emit(name, runs["device_wgrads"], runs["torch_wgrads"], parameters=sum(p.numel() for p in base.parameters()), changed=changed)

    name, B, T, idim, hdim = "train_step_gru_yaml_256x100", 256, 100, 40, 128
    if a.only in name:
        batch = dict(feats=t((B, T, idim)), target=torch.from_numpy(rng.integers(-1, 1, (B, 1)).astype(np.int64)).to(dev),
                     feats_lengths=torch.from_numpy(rng.integers(T // 2, T + 1, B).astype(np.int32)).to(dev),
                     target_lengths=torch.ones(B, dtype=torch.int32, device=dev))
        torch.manual_seed(0)
        base = Kws(idim, hdim, 1, nn.GRU(hdim, hdim, num_layers=2, batch_first=True))
        step_pair(name, base, batch, {"criterion": "max_pooling", "grad_clip": 5.0, "log_interval": 1 << 30}, dg.use_device_grus,
                  lr=1e-3, weight_decay=5e-5)

    name, Lmax = "train_step_fsmn_ctc_256x100", 6
    if a.only in name:
        batch = dict(feats=t((B, T, 400)), target=torch.from_numpy(rng.integers(1, 2599, (B, Lmax)).astype(np.int64)).to(dev),
                     feats_lengths=torch.from_numpy(rng.integers(60, T + 1, B).astype(np.int32)).to(dev),
                     target_lengths=torch.from_numpy(rng.integers(3, Lmax + 1, B).astype(np.int32)).to(dev))
        torch.manual_seed(0)
        step_pair(name, fsmn.FSMN(*CTC), batch, {"criterion": "ctc", "grad_clip": 5.0, "log_interval": 1 << 30}, lambda m: 0,
                  lr=1e-3, weight_decay=1e-4)

    name = "units_gru_recipe"
    if a.only in name:
        import json
        from tests import gru_train_matrix as gm
        out = dict(name=name, bars={q: gm.BARS[q] for q in ("dw_ih", "dw_hh", "db_ih", "db_hh")})
        for switch in (False, True):
            m = gm.module("recipe", cls=dg.DeviceGRU, device="cuda")
            m.device_weight_grads = switch
            u, bad = gm.units("recipe", gm.run_module("recipe", m, device="cuda"))
            assert not bad, bad
            out["device_weight_grads" if switch else "rocblas_weight_grads"] = {q: round(u[q], 2) for q in out["bars"]}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
