#!/usr/bin/env python3
"""Measurement: the validation criterion on the device (wekws_amd.criterion) beside the model forward of the same batch.

    max_pooling  (1024, 98, 2) and (8192, 98, 2)      forward: ds_tcn_h256, 98 frames
    ctc          (256, 100, 2599), 8 labels per row, with and without the utterance accuracy      forward: ds_tcn_h256_ctc
    ce           (8192, 12)                            forward: mdtc_h64_global12, 98 frames

Timing as tools/bench_configs.py::timeit: warm-up of every shape, 0.3 s of work first (an idle device starts at lower
clocks), then the median / p10 / p90 of 30 groups of 10 back-to-back calls between two device events.  GPU only; one JSON
line per measurement, the host figures of the reference's criterion (one process on a build machine's CPU, random inputs:
max_pooling 375 ms at (1024, 98, 2), ctc 640 ms at (256, 100, 2599) without accuracy) repeated beside them.

    python tools/probe/criterion_step.py > criterion_step.jsonl"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tools.bench_configs import build, timeit  # noqa: E402
from wekws_amd import criterion as crit  # noqa: E402
from wekws_amd.utils import synth  # noqa: E402

CPU_REFERENCE_MS = {"max_pooling_1024x98x2": 375.0, "ctc_256x100x2599": 640.0}


def line(name, fn, fwd_ms=None, **extra):
    med, p10, p90 = timeit(fn)
    rec = dict(name=name, ms=round(med, 4), p10=round(p10, 4), p90=round(p90, 4), **extra)
    if fwd_ms is not None:
        rec["forward_ms"] = round(fwd_ms, 4)
        rec["criterion_over_forward"] = round(med / fwd_ms, 3)
    if name in CPU_REFERENCE_MS:
        rec["reference_cpu_ms"] = CPU_REFERENCE_MS[name]
        rec["speedup_over_reference_cpu"] = round(CPU_REFERENCE_MS[name] / med, 1)
    print(json.dumps(rec), flush=True)
    return med


def main():
    assert torch.cuda.is_available(), "criterion_step.py measures on the GPU only"
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)

    cfg, m = build("ds_tcn_h256")
    for B in (1024, 8192):
        x = torch.from_numpy(synth.synth_feats(B, 98, cfg["input_dim"], seed=1)).to(dev)
        fwd = line(f"forward_ds_tcn_h256_{B}x98", lambda: m(x))
        scores = m(x)[0]
        tg = torch.from_numpy(rng.integers(-1, 2, B).astype(np.int32)).to(dev)
        ln = torch.from_numpy(rng.integers(50, 99, B).astype(np.int32)).to(dev)
        line(f"max_pooling_{B}x98x2", lambda: crit.max_pooling_loss_device(scores, tg, ln, 0), fwd)
    del m

    cfg, m = build("ds_tcn_h256_ctc")
    B, T, V, S = 256, 100, 2599, 8
    x = torch.from_numpy(synth.synth_feats(B, T, cfg["input_dim"], seed=2)).to(dev)
    fwd = line(f"forward_ds_tcn_h256_ctc_{B}x{T}", lambda: m(x))
    logits = torch.from_numpy((rng.standard_normal((B, T, V)) * 2).astype(np.float32)).to(dev)
    tg = torch.from_numpy(rng.integers(1, V, (B, S)).astype(np.int32)).to(dev)
    ln = torch.full((B,), T, dtype=torch.int32, device=dev)
    tl = torch.full((B,), S, dtype=torch.int32, device=dev)
    line(f"ctc_{B}x{T}x{V}", lambda: crit.ctc_loss_device(logits, tg, ln, tl, False), fwd, labels=S)
    line(f"ctc_acc_{B}x{T}x{V}", lambda: crit.ctc_loss_device(logits, tg, ln, tl, True), fwd, labels=S)
    # peaked posteriors (a trained model's): the decode keeps one or two candidates per frame instead of none
    peaked = logits.clone()
    peaked[torch.arange(B, device=dev)[:, None], torch.arange(T, device=dev)[None, :],
           torch.from_numpy(rng.integers(0, V, (B, T))).to(dev)] = 20.0
    line(f"ctc_acc_peaked_{B}x{T}x{V}", lambda: crit.ctc_loss_device(peaked, tg, ln, tl, True), fwd, labels=S)
    del m

    cfg, m = build("mdtc_h64_global12")
    B = 8192
    x = torch.from_numpy(synth.synth_feats(B, 98, cfg["input_dim"], seed=3)).to(dev)
    fwd = line(f"forward_mdtc_h64_global12_{B}x98", lambda: m(x))
    lg = m(x)[0]
    tg = torch.from_numpy(rng.integers(0, 12, B).astype(np.int32)).to(dev)
    line(f"ce_{B}x12", lambda: crit.cross_entropy_device(lg, tg), fwd)


if __name__ == "__main__":
    main()
