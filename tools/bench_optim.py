#!/usr/bin/env python3
"""Measurement: the last three statements of a training step -- clip_grad_norm_, the finite test, Adam.step() -- at the
parameter shapes of the DS-TCN h256 and of fsmn_ctc (the state dicts wekws_amd/pack.py reads, filled with seeded noise), three
variants alternated in one process:

    torch        clip_grad_norm_(params, 5); if torch.isfinite(norm): optim.Adam(...).step()      (the reference's statements)
    torch_fused  the same with optim.Adam(..., fused=True)
    clip_adam    wekws_amd.optim.ClipAdam.clip_and_step(5)                                       (three launches, no host read)

and one full TrainExecutor step (forward, criterion, backward, clip, step) of a small torch module with torch's Adam and with
ClipAdam.  Timing: warm-up, 0.3 s of work first, then per variant and round 10 groups of 10 back-to-back steps between two
device events; the variants take turns over 3 rounds and the line carries median / p10 / p90 of a variant's 30 groups.  The
reference's `if` reads the norm on the host, so its steps cannot queue up: the time between the events is then the host's.

Kernel times and launches per step come from separate `rocprofv3 --kernel-trace --stats` runs of `--run VARIANT --steps N`
(one variant, N steps, data made on the host so that set-up launches nothing): with `--traces DIR` holding
DIR/<model>_<variant>_<N>/**/*kernel_stats.csv for N = 20 and 120, the line carries the difference of the two runs per step.
Bytes per step from the shapes: p, g, m, v read and p, m, v written (28 B an element) plus the norm's read of g (4 B).
GPU only; one JSON line per measurement.

    python tools/bench_optim.py [--traces DIR] > profiles/optim_step.jsonl"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch
from torch.nn.utils import clip_grad_norm_

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wekws_amd import pack  # noqa: E402
from wekws_amd.optim import ClipAdam  # noqa: E402
from wekws_amd.utils import synth  # noqa: E402

HBM_PEAK = 8.0e12
HYPER = dict(lr=1e-3, weight_decay=1e-4)
CLIP = 5.0
MODELS = ("ds_tcn_h256", "fsmn_ctc")
VARIANTS = ("torch", "torch_fused", "clip_adam")
NOT_PARAMETERS = ("running_mean", "running_var", "num_batches_tracked", "global_cmvn")


def param_shapes(model):
    """Shapes of the model's trainable tensors, in state_dict order (buffers left out)."""
    return [tuple(s) for n, s in pack.model_spec(synth.MODEL_CONFIGS[model]) if not any(k in n for k in NOT_PARAMETERS)]


def make_variant(model, variant, dev):
    """-> (step function, element count, tensors): parameters and gradients of seeded noise made on the host."""
    rng = np.random.default_rng(11)
    shapes = param_shapes(model)
    ps = [torch.nn.Parameter(torch.from_numpy((0.1 * rng.standard_normal(s)).astype(np.float32)).to(dev)) for s in shapes]
    gs = [torch.from_numpy((0.01 * rng.standard_normal(s)).astype(np.float32)).to(dev) for s in shapes]
    n = sum(p.numel() for p in ps)
    if variant == "clip_adam":
        opt = ClipAdam(ps, **HYPER)
        for p, g in zip(ps, gs):
            p.grad.copy_(g)
        return (lambda: opt.clip_and_step(CLIP)), n, len(ps)
    for p, g in zip(ps, gs):
        p.grad = g
    opt = torch.optim.Adam(ps, fused=(variant == "torch_fused"), **HYPER)

    def step():
        norm = clip_grad_norm_(ps, CLIP)
        if torch.isfinite(norm):
            opt.step()
    return step, n, len(ps)


def groups(fn, reps=10, group=10):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(group):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / group)
    return ts


def alternate(fns, rounds=3):
    """{name: samples}: every function warmed up, then the functions take turns."""
    import time
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()             # an idle MI355X runs its first ~0.25 s of work at lower clocks: measure behind that
    while time.perf_counter() - t0 < 0.3:
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k] += groups(fn)
    return out


def stats_of(root, model, variant, steps):
    """{kernel: (calls, total ns)} of the run's kernel-stats CSV, or None."""
    found = glob.glob(os.path.join(root, f"{model}_{variant}_{steps}", "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        return None
    out = {}
    with open(found[0]) as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = (int(row["Calls"]), float(row["TotalDurationNs"]))
    return out


def trace_fields(root, model, variant):
    a, b = stats_of(root, model, variant, 20), stats_of(root, model, variant, 120)
    if not a or not b:
        return {}
    calls = sum(c for c, _ in b.values()) - sum(c for c, _ in a.values())
    ns = sum(t for _, t in b.values()) - sum(t for _, t in a.values())
    out = dict(launches_per_step=round(calls / 100, 2), kernel_us_per_step=round(ns / 100 / 1e3, 2))
    if variant == "clip_adam":
        for k in ("grad_sumsq_kernel", "clip_fold_kernel", "adam_apply_kernel"):
            for name, (c, t) in b.items():
                if k in name:
                    out[k + "_us"] = round(t / c / 1e3, 2)
    return out


class SmallNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(40, 256)
        self.b = torch.nn.Linear(256, 256)
        self.c = torch.nn.Linear(256, 2)

    def forward(self, x):
        return torch.sigmoid(self.c(torch.relu(self.b(torch.relu(self.a(x)))))), None


def executor_steps(dev):
    from wekws_amd.utils.executor import TrainExecutor
    rng = np.random.default_rng(12)
    B, T, nb = 256, 98, 10
    loader = [dict(feats=torch.from_numpy(rng.standard_normal((B, T, 40)).astype(np.float32)).to(dev),
                   target=torch.from_numpy(rng.integers(-1, 2, (B, 1))).to(dev),
                   feats_lengths=torch.from_numpy(rng.integers(T // 2, T + 1, B).astype(np.int32)).to(dev),
                   target_lengths=torch.ones(B, dtype=torch.int32, device=dev)) for _ in range(nb)]
    args = {"criterion": "max_pooling", "min_duration": 0, "grad_clip": CLIP, "log_interval": 1000}
    fns = {}
    for name in ("torch", "clip_adam"):
        torch.manual_seed(13)
        net = SmallNet().to(dev)
        opt = ClipAdam(net.parameters(), **HYPER) if name == "clip_adam" else torch.optim.Adam(net.parameters(), **HYPER)
        fns[name] = (lambda net=net, opt=opt: TrainExecutor().train(net, opt, loader, dev, None, args))
    n = sum(p.numel() for p in SmallNet().parameters())
    for name, ts in alternate(fns).items():
        ts = np.array(ts) / nb
        print(json.dumps(dict(name=f"train_executor_step_smallnet_B{B}xT{T}", optimizer=name, elements=n, ms=round(float(np.median(ts)), 4),
                              p10=round(float(np.percentile(ts, 10)), 4), p90=round(float(np.percentile(ts, 90)), 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", default=None, help="directory of the rocprofv3 runs (see the module docstring)")
    ap.add_argument("--run", default=None, choices=VARIANTS, help="run --steps steps of one variant and exit (under rocprofv3)")
    ap.add_argument("--model", default="ds_tcn_h256", choices=MODELS)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_optim.py measures on the GPU only"
    dev = torch.device("cuda", 0)
    if a.run:
        fn, _, _ = make_variant(a.model, a.run, dev)
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return
    for model in MODELS:
        made = {v: make_variant(model, v, dev) for v in VARIANTS}
        n, tensors = made["torch"][1], made["torch"][2]
        for v, ts in alternate({v: m[0] for v, m in made.items()}).items():
            med = float(np.median(ts))
            line = dict(name=f"optim_step_{model}", variant=v, tensors=tensors, elements=n, bytes_per_step=32 * n, ms=round(med, 4),
                        p10=round(float(np.percentile(ts, 10)), 4), p90=round(float(np.percentile(ts, 90)), 4))
            if a.traces:
                line.update(trace_fields(a.traces, model, v))
                if "kernel_us_per_step" in line and line["kernel_us_per_step"] > 0:
                    line["kernel_share_of_hbm_peak"] = round(32 * n / (line["kernel_us_per_step"] * 1e-6) / HBM_PEAK, 4)
            print(json.dumps(line), flush=True)
    executor_steps(dev)


if __name__ == "__main__":
    main()
