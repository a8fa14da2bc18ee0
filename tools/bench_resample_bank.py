#!/usr/bin/env python3
"""Measurements of the rate bank (wekws_amd.frontend.StreamingResamplerBank), one JSON line each; not the bench.py contract.
GPU only.

    python tools/bench_resample_bank.py --out profiles/resample_bank.jsonl

(a) a one-member bank (48000) against StreamingResampler(4096, 48000): 4096 streams x 14400 samples (0.3 s) per push.
(b) 4096 streams in thirds over 8000 / 16000 / 48000 with 0.3 s per push each (2400 / 4800 / 14400 samples): ONE bank push against
    the three single-rate pushes of the same rows queued back to back on one stream.
Both sides of a comparison run in the same process in steady state (every stream holds its history), int16 out, with the same
row capacity, and alternate: a repetition times a group of pushes of one side, then of the other, between device events behind
a warm-up.  Each record gives the median and p10 ... p90 of both sides and the ratio of the medians."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wekws_amd.frontend import StreamingResampler, StreamingResamplerBank  # noqa: E402

B = 4096


def time_pair(fa, fb, warm=3, reps=20, group=10):
    """median, p10, p90 in ms per call of fa and of fb, alternating groups of calls"""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    t_pre = time.perf_counter()                 # an idle MI355X runs its first ~0.25 s of work at lower clocks
    while time.perf_counter() - t_pre < 0.3:
        for _ in range(group):
            fa()
            fb()
        torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(reps):
        for side, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(group):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts[side].append(a.elapsed_time(b) / group)
    return [(float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))) for t in ts]


def record(kind, config, bank, single, **kw):
    row = dict(kind=kind, config=config, B=B, **kw)
    for name, (med, p10, p90) in (("bank", bank), ("single", single)):
        row.update({f"ms_{name}": round(med, 4), f"{name}_p10": round(p10, 4), f"{name}_p90": round(p90, 4)})
    row["bank_over_single"] = round(bank[0] / single[0], 3)
    row["within_single_spread"] = bool(single[1] <= bank[0] <= single[2])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_resample_bank.py measures on the GPU; none is visible")
    g = torch.Generator(device="cuda").manual_seed(7)
    n = 14400
    x = torch.randint(-20000, 20000, (B, n), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
    out = []

    # ---- (a) one member
    one = StreamingResampler(B, 48000, 16000, max_chunk=n)
    bank = StreamingResamplerBank(B, [48000], 16000, max_chunk=n)
    cap = one.max_out(n)
    assert bank.max_out(n) == cap
    for _ in range(2):                                              # steady state: every stream holds its history
        ya, ca = bank.push(x, capacity=cap)
        yb, cb = one.push(x, capacity=cap)
    assert ca == cb and torch.equal(ya, yb)
    tb, ts = time_pair(lambda: bank.push(x, capacity=cap), lambda: one.push(x, capacity=cap))
    out.append(record("resample_bank", "(a) one member 48000 vs StreamingResampler(48000)", tb, ts, chunk=n, capacity=cap,
                      samples_per_push=int(ca[0])))
    del one, bank

    # ---- (b) thirds over three rates
    rates, lens, cuts = (8000, 16000, 48000), (2400, 4800, 14400), (0, 1365, 2730, B)
    bank = StreamingResamplerBank(B, rates, 16000, max_chunk=n)
    singles, parts = [], []
    for m, rate in enumerate(rates):
        a, b = cuts[m], cuts[m + 1]
        bank.set_rate(range(a, b), rate)
        singles.append(StreamingResampler(b - a, rate, 16000, max_chunk=lens[m]))
        parts.append(x[a:b, :lens[m]].contiguous())
    cap = max(rs.max_out(k) for rs, k in zip(singles, lens))
    samples = np.asarray([lens[m] for m in range(3) for _ in range(cuts[m], cuts[m + 1])], dtype=np.int32)

    def three():
        return [rs.push(p, capacity=cap) for rs, p in zip(singles, parts)]

    for _ in range(2):
        ya, ca = bank.push(x, samples=samples, capacity=cap)
        ys = three()
    assert ca == [c for _, cs in ys for c in cs] and torch.equal(ya, torch.cat([y for y, _ in ys]))
    tb, ts = time_pair(lambda: bank.push(x, samples=samples, capacity=cap), three)
    out.append(record("resample_bank", "(b) thirds 8000/16000/48000: one bank push vs three single-rate pushes", tb, ts,
                      chunk=list(lens), capacity=cap, samples_per_push=int(ca[0])))
    if args.out:
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
