#!/usr/bin/env python3
"""The streaming MODEL STEP for many streams, measured three ways (one JSON line each, not the bench.py contract).  GPU only.

    python tools/bench_stream_step.py [--streams 4096] [--rounds 12] [--group 4] [model ...]  > profiles/stream_step.jsonl

Per model (default: ds_tcn_h256, the headline DS-TCN, and fsmn_ctc300, the small CTC FSMN), `streams` streams with one resident
chunk each, inputs on the device:
  (a)   the bucketed step BatchedKeyWordSpotter.forward made before forward_streams: per bucket of equal frame count
        index_select of the features and caches out of a dense pool tensor, KWSModel.forward, index_copy_ back;
  (b)   KWSModel.forward_streams over a StreamCachePool, 10 frames in every row         -- against (a) with one bucket;
  (c)   the same with frames cycling 9 / 10 / 11                                       -- against (a) bucketed three ways;
  (u)   KWSModel.forward on (streams, 10) with a dense cache: the existing uniform streaming step (the stream4096 probe's case).
The variants are interleaved round by round in ONE process; a figure is the median over the rounds of `group` back-to-back steps
between two device events.  (a) is measured twice per round (a1, a2, and a3x twice: a3x1, a3x2): the difference of their medians is the
run-to-run spread every comparison is held against.  Bytes: a stream's cache is cache_elems x 4 B; the kernel reads and writes the
pool once (2 x), (a) moves it six times."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wekws_amd import pack  # noqa: E402
from wekws_amd.model.kws_model import StreamCachePool, init_model  # noqa: E402
from wekws_amd.utils import synth  # noqa: E402

TCAP = 11


def build(name):
    cfg = dict(synth.MODEL_CONFIGS[name])
    m = init_model(cfg)
    sd = synth.synth_state_dict(pack.model_spec(cfg), 1234)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return cfg, m.cuda().eval().freeze()


def bucketed(model, dense, x, buckets, softmax):
    """(a): `buckets` = [(frames, row index tensor)]; the rows are the streams."""
    fwd = model.forward_softmax if softmax else model.forward
    for n, idx in buckets:
        y, c = fwd(x.index_select(0, idx)[:, :n].contiguous(), dense.index_select(0, idx).contiguous())
        dense.index_copy_(0, idx, c)
    return y


def measure(name, streams, rounds, group):
    cfg, model = build(name)
    softmax = cfg.get("activation", {}).get("type") == "identity"         # the CTC heads run forward_softmax
    dev = torch.device("cuda")
    x = torch.from_numpy(synth.synth_feats(streams, TCAP, cfg["input_dim"], seed=1)).to(dev)
    x10 = x[:, :10].contiguous()
    ids = np.arange(streams, dtype=np.int32)
    f10, f3 = np.full(streams, 10, dtype=np.int32), (9 + ids % 3).astype(np.int32)
    all_rows = torch.arange(streams, device=dev)
    three = [(n, torch.from_numpy(np.flatnonzero(f3 == n)).to(dev)) for n in (9, 10, 11)]
    dense = torch.zeros(pack.cache_shape(model._d, streams), dtype=torch.float32, device=dev)
    carried = [torch.zeros_like(dense)]
    pool = StreamCachePool(model, streams)
    run = model.forward_softmax_streams if softmax else model.forward_streams
    fwd = model.forward_softmax if softmax else model.forward
    ybuf = torch.empty((streams, TCAP, model.odim), dtype=torch.float32, device=dev)
    y10 = torch.empty((streams, 10, model.odim), dtype=torch.float32, device=dev)

    def uniform():
        carried[0] = fwd(x10, carried[0])[1]

    variants = {
        "a1": lambda: bucketed(model, dense, x, [(10, all_rows)], softmax),
        "b": lambda: run(x10, f10, ids, pool, out=y10),
        "a3x1": lambda: bucketed(model, dense, x, three, softmax),
        "c": lambda: run(x, f3, ids, pool, out=ybuf),
        "u": uniform,
        "a2": lambda: bucketed(model, dense, x, [(10, all_rows)], softmax),
        "a3x2": lambda: bucketed(model, dense, x, three, softmax),
    }
    for fn in variants.values():                                           # every shape warm
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()                 # an idle MI355X runs its first ~0.25 s of work at lower clocks: measure behind that
    while time.perf_counter() - t0 < 0.5:
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(group):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) / group)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    cache_bytes = dense.numel() * 4
    rec = dict(kind="stream_step", model=name, streams=streams, rounds=rounds, group=group, softmax=bool(softmax),
               pool_MB=round(cache_bytes / 1e6, 1), ms={k: round(v, 4) for k, v in med.items()},
               p10={k: round(float(np.percentile(v, 10)), 4) for k, v in ts.items()},
               p90={k: round(float(np.percentile(v, 90)), 4) for k, v in ts.items()},
               spread_ms=round(max(abs(med["a1"] - med["a2"]), abs(med["a3x1"] - med["a3x2"])), 4),
               b_over_a=round(med["b"] / min(med["a1"], med["a2"]), 4), c_over_a3=round(med["c"] / min(med["a3x1"], med["a3x2"]), 4),
               b_over_u=round(med["b"] / med["u"], 4),
               kernel_GBps_at_b=round(2 * cache_bytes / med["b"] / 1e6, 1), device=torch.cuda.get_device_name(0))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--group", type=int, default=4)
    ap.add_argument("models", nargs="*", default=["ds_tcn_h256", "fsmn_ctc300"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stream_step.py measures on the GPU only"
    for name in args.models:
        measure(name, args.streams, args.rounds, args.group)


if __name__ == "__main__":
    main()
