#!/usr/bin/env python3
"""Measurements of the augmentation stages (wekws_amd.augment), one JSON line each; not the bench.py contract.  GPU only.

    python tools/bench_augment.py --out profiles/augment.jsonl

Reverberation at B = 1024: 1-s utterances with 64 RIRs of 8000 and of 16000 taps, 4-s utterances with 16000 taps, and -- to
split the cost -- the same rows with one-tap RIRs (one partition: both transforms and a single product per bin, no block sum
beyond it).  Beside them the noise mix, the masks, a fbank call, the chain Resample(48000) -> Reverb -> AddNoise -> Fbank, and
one row of scipy.signal.convolve on one host thread.  Times are device events around groups of back-to-back calls behind a
warm-up (median, p10, p90); `bytes` is what the stage must move by its definition (computed from the shapes below), and
`hbm_fraction` that over 8 TB/s over the measured time."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wekws_amd.augment import AddNoise, Reverb, spec_aug  # noqa: E402
from wekws_amd.frontend import Fbank, Resample  # noqa: E402

HBM = 8.0e12


def timeit(fn, warm=3, reps=20, group=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t_pre = time.perf_counter()                 # an idle MI355X runs its first ~0.25 s of work at lower clocks
    while time.perf_counter() - t_pre < 0.3:
        for _ in range(group):
            fn()
        torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(group):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / group)
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def rirs(count, taps, seed=0):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((count, taps)) * np.exp(-6.9 * np.arange(taps) / max(taps, 2))[None, :]
    h[:, 0] = 1.0
    return np.round(h * 20000.0).astype(np.float32)


def row(out, **kw):
    if "ms" in kw and "bytes" in kw:
        kw["ms_at_8TBs"] = round(kw["bytes"] / HBM * 1e3, 4)
        kw["hbm_fraction"] = round(kw["bytes"] / HBM * 1e3 / kw["ms"], 3)
    out.append(kw)
    print(json.dumps(kw), flush=True)


def reverb_bytes(B, n, taps, hop):
    """forward: the samples in, the spectra out; inverse: per block the spectra of min(P, b + 1) input blocks and as many
    partitions of the RIR in, the samples out"""
    nb, P, bins = -(-n // hop), -(-taps // hop), hop + 1
    products = sum(min(P, b + 1) for b in range(nb))
    return B * (n * 4 + nb * bins * 8) + B * (products * 2 * bins * 8 + n * 4), B * products * bins * 8


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="", help="also write the rows to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_augment.py measures on the GPU only"
    dev = "cuda"
    out = []
    B = 1024
    g = torch.Generator().manual_seed(0)
    for n, taps, R in ((16000, 8000, 64), (16000, 16000, 64), (64000, 16000, 64), (16000, 1, 64), (64000, 1, 64)):
        pcm = (torch.rand((B, n), generator=g) * 2 - 1).to(dev)
        rv = Reverb(rirs(R, taps))
        pick = np.arange(B) % R
        dst = torch.empty_like(pcm)
        med, p10, p90 = timeit(lambda: rv(pcm, pick, out=dst))
        nbytes, flops8 = reverb_bytes(B, n, taps, rv.hop)
        row(out, kind="reverb", B=B, samples=n, taps=taps, rirs=R, partitions=-(-taps // rv.hop), blocks=-(-n // rv.hop), ms=round(med, 4),
            p10=round(p10, 4), p90=round(p90, 4), bytes=nbytes, block_sum_gflop=round(flops8 / 1e9, 3), utt_per_s=round(B / med * 1e3),
            spectra_mb=round(rv.spectra_bytes / 2 ** 20, 2), workspace_mb=round(rv.workspace_bytes(B, n) / 2 ** 20, 1))
        del rv, pcm, dst
    n = 16000
    pcm = (torch.rand((B, n), generator=g) * 2 - 1).to(dev)
    rng = np.random.default_rng(1)
    nz = AddNoise(np.round(rng.standard_normal((16, 160000)) * 2500.0).astype(np.float32), pcm_scale=1.0)
    which, start, snr = np.arange(B) % 16, (977 * np.arange(B)) % 140000, (np.arange(B) % 16).astype(np.float64)
    dst = pcm.clone()
    med, p10, p90 = timeit(lambda: nz(dst, which, start, snr, inplace=True))
    row(out, kind="noise_mix", B=B, samples=n, ms=round(med, 4), p10=round(p10, 4), p90=round(p90, 4), bytes=3 * B * n * 4)
    fb = Fbank(80)
    pcm16 = pcm * 32768.0
    med, p10, p90 = timeit(lambda: fb(pcm16))
    row(out, kind="fbank80", B=B, samples=n, ms=round(med, 4), p10=round(p10, 4), p90=round(p90, 4))
    feats = fb(pcm16)
    T, F = int(feats.size(1)), int(feats.size(2))
    tm = np.stack([np.asarray([[b % 40, b % 40 + 30], [60, 90]]) for b in range(B)]).astype(np.int32)
    fm = np.stack([np.asarray([[b % 70, b % 70 + 8], [3, 9]]) for b in range(B)]).astype(np.int32)
    med, p10, p90 = timeit(lambda: spec_aug(feats, tm, fm, inplace=True))
    row(out, kind="spec_mask", B=B, frames=T, bins=F, ms=round(med, 4), p10=round(p10, 4), p90=round(p90, 4), bytes=2 * B * T * F * 4)
    # the chain of a training batch that arrives at 48 kHz
    raw = (torch.rand((B, 48000), generator=g) * 2 - 1).to(dev)
    rs = Resample(48000)
    rv = Reverb(rirs(64, 8000))
    pick = np.arange(B) % 64

    def chain():
        x = rs(raw)
        y = nz(rv(x, pick), which, start, snr, inplace=True)
        return fb(y * 32768.0)

    med, p10, p90 = timeit(chain)
    row(out, kind="chain resample48k-reverb8000-noise-fbank80", B=B, ms=round(med, 4), p10=round(p10, 4), p90=round(p90, 4),
        utt_per_s=round(B / med * 1e3))
    med_rs, _, _ = timeit(lambda: rs(raw))
    row(out, kind="resample48k", B=B, ms=round(med_rs, 4))
    # the host path this replaces: one row on one thread
    from scipy import signal
    x = raw[0, :16000].cpu().numpy()
    for taps in (8000, 16000):
        h = rirs(1, taps)[0]
        h = h / np.sqrt(np.sum(h ** 2))
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            signal.convolve(x, h, mode="full")[:x.size]
            ts.append(time.perf_counter() - t0)
        row(out, kind="scipy.signal.convolve, one row, one thread", samples=16000, taps=taps, ms=round(float(np.median(ts)) * 1e3, 4))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
