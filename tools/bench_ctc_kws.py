#!/usr/bin/env python3
"""Times the on-device CTC prefix beam search and keyword detection (wekws_amd.ctc) on one GPU and the host oracle
(tests/ctc_kws_ref.py) on one CPU core; prints one JSON record per row, and writes them as a list to --out if given.

    timeout -k 10 600 python tools/bench_ctc_kws.py [--out records.json]

Rows: the offline search of 4096 utterances x 98 frames x 2599 tokens; 4096 streams in 30-frame chunks; the latency of
one 30-frame chunk of one stream; the host oracle on one utterance / one chunk."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ctc_kws_ref as R  # noqa: E402
from wekws_amd import ctc  # noqa: E402

KWS = [(3, 4, 5), (3, 6, 7)]


def peaky(g, B, T, V):
    x = torch.randn(B, T, V, generator=g)
    dom = torch.randint(0, 8, (B, T), generator=g) * (torch.rand(B, T, generator=g) < .35)
    x.scatter_add_(2, dom.unsqueeze(2), torch.full((B, T, 1), 7.0))
    return x.softmax(2)


def gpu_time(fn, warmup=3, iters=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the records to this JSON file")
    args = ap.parse_args()
    g = torch.Generator().manual_seed(1)
    V, B, T = 2599, 4096, 98
    probs = peaky(g, B, T, V).cuda()
    out = []
    ms = gpu_time(lambda: ctc.keyword_search(probs, None, KWS))
    out.append(dict(row="offline_search", B=B, T=T, V=V, ms=ms, utt_per_s=B / ms * 1e3,
                    hbm_gb=B * T * V * 4 / 1e9))
    sp = ctc.StreamingKeywordSpotter(B, KWS, 0.5, vocab=V)
    chunk = probs[:, :30].contiguous()
    ms = gpu_time(lambda: sp.step_records(chunk))
    out.append(dict(row="stream_chunk30", B=B, V=V, ms=ms, streams_per_s=B / ms * 1e3))
    one = ctc.StreamingKeywordSpotter(1, KWS, 0.5, vocab=V)
    c1 = chunk[:1].contiguous()
    ms = gpu_time(lambda: one.step_records(c1), iters=50)
    out.append(dict(row="stream_chunk30_B1_latency", ms=ms))
    host = probs[:1].cpu().numpy()
    t0 = time.perf_counter()
    R.keyword_search(host[0], KWS, 3, 20, R.default_tokenset(KWS))
    t_utt = (time.perf_counter() - t0) * 1e3
    o = R.Spotter(KWS, 0.5)
    t0 = time.perf_counter()
    o.step(host[0, :30])
    t_chunk = (time.perf_counter() - t0) * 1e3
    out.append(dict(row="host_oracle_one_core", utterance_ms=t_utt, chunk30_ms=t_chunk))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for r in out:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
