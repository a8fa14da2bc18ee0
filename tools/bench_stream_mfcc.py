#!/usr/bin/env python3
"""The streaming front end's push in log-mel and in MFCC mode, and the streaming threshold detector's step (one JSON line each, not
the bench.py contract).  GPU only.

    python tools/bench_stream_mfcc.py [--streams 4096] [--rounds 20] [--group 4] [--fbank-only] [--root DIR]

push      the `p80` front end (80 bins, Povey window, no context), `streams` streams, one 4,800-sample chunk each (30 frames per
          stream in the steady state), interleaved round by round in ONE process:
            fb1, fb2   log-mel mode, measured twice per round: the difference of their medians is the run-to-run spread
            mfcc       MFCC mode (80 cepstra, lifter 22): the DCT in the fbank kernel's epilogue
            fb_dct     what it replaces: the log-mel push plus one wekws_hip_dct_lifter launch over the push's rows
          --fbank-only measures fb1 / fb2 alone; with --root DIR the package of another checkout (a parent commit built beside this
          one) is measured, for a same-session comparison of the log-mel mode across the two.
detector  wekws_hip_threshold_kws_step for streams x 10 frames x 2 keywords (threshold; threshold_py: the same through
          StreamingThresholdSpotter.step_records, allocations included), next to wekws_hip_ctc_kws_step for the same rows (a 2-class
          vocabulary, one keyword of one token).  For the record only: the two do different work.
A figure is the median over the rounds of `group` back-to-back calls between two device events."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NSAMP, FB = 4800, dict(num_bins=80, window="povey")


def timed(variants, rounds, group):
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
    return ({k: round(float(np.median(v)), 4) for k, v in ts.items()},
            {k: round(float(np.percentile(v, 10)), 4) for k, v in ts.items()},
            {k: round(float(np.percentile(v, 90)), 4) for k, v in ts.items()})


def measure_push(args, root):
    from wekws_amd.frontend import StreamingFrontEnd
    g = torch.Generator(device="cuda").manual_seed(1)
    pcm = torch.randint(-20000, 20000, (args.streams, NSAMP), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
    fb = StreamingFrontEnd(args.streams, max_chunk=NSAMP, **FB)
    cap = fb.max_frames(NSAMP)
    out_fb = torch.zeros((args.streams, cap, 80), dtype=torch.float32, device="cuda")
    variants = {"fb1": lambda: fb.push(pcm, out=out_fb)}
    if not args.fbank_only:
        from wekws_amd.frontend import dct_lifter
        mf = StreamingFrontEnd(args.streams, max_chunk=NSAMP, num_ceps=80, cepstral_lifter=22.0, **FB)
        fb3 = StreamingFrontEnd(args.streams, max_chunk=NSAMP, **FB)
        out_mf, out_3 = torch.zeros_like(out_fb), torch.zeros_like(out_fb)
        variants["mfcc"] = lambda: mf.push(pcm, out=out_mf)

        def fb_dct():
            _, frames = fb3.push(pcm, out=out_3)
            return dct_lifter(out_3[:, :frames[0]], 80, 22.0)

        variants["fb_dct"] = fb_dct
    variants["fb2"] = variants["fb1"]
    med, p10, p90 = timed(variants, args.rounds, args.group)
    rec = dict(kind="stream_push", root=os.path.relpath(root, ROOT), streams=args.streams, nsamp=NSAMP, rounds=args.rounds, group=args.group,
               ms=med, p10=p10, p90=p90, spread_ms=round(abs(med["fb1"] - med["fb2"]), 4), device=torch.cuda.get_device_name(0))
    if not args.fbank_only:
        a, b = out_mf.clone(), dct_lifter(out_3, 80, 22.0)
        # (both handles are in the steady state: the same 30 frames per stream; bit-identity is what tests/test_hip_stream_mfcc.py holds)
        rec["mfcc_equals_fb_dct_bits"] = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
        rec["mfcc_over_fb_dct"] = round(med["mfcc"] / med["fb_dct"], 4)
        rec["mfcc_minus_fb_ms"] = round(med["mfcc"] - min(med["fb1"], med["fb2"]), 4)
    print(json.dumps(rec), flush=True)


def measure_detector(args):
    from wekws_amd.ctc import StreamingKeywordSpotter
    from wekws_amd.det import StreamingThresholdSpotter
    T, K = 10, 2
    g = torch.Generator(device="cuda").manual_seed(2)
    probs = torch.rand((args.streams, T, K), device="cuda", generator=g)
    soft = torch.softmax(probs * 4, dim=2).contiguous()
    thr = StreamingThresholdSpotter(args.streams, ["a", "b"], 0.9, window_shift=50)
    ctc = StreamingKeywordSpotter(args.streams, {"a": (1,)}, 0.5, vocab=K)
    ids = torch.arange(args.streams, dtype=torch.int32, device="cuda")
    fr = torch.full((args.streams,), T, dtype=torch.int32, device="cuda")
    res = torch.empty((args.streams, 32), dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib, h = ctc._hd.lib, ctc._hd.h
    D = thr._lib.wekws_hip_threshold_kws_max_hits(thr._ptr, T)
    hf = torch.empty((args.streams, K, D), dtype=torch.int32, device="cuda")
    hs = torch.empty((args.streams, K, D), dtype=torch.float32, device="cuda")
    best = torch.empty((args.streams, K), dtype=torch.float32, device="cuda")
    bf = torch.empty((args.streams, K), dtype=torch.int32, device="cuda")
    st = torch.empty((args.streams,), dtype=torch.int32, device="cuda")
    variants = {
        # the C entry points alone, then the Python call with its allocations
        "threshold": lambda: thr._lib.wekws_hip_threshold_kws_step(thr._ptr, probs.data_ptr(), args.streams, T, ids.data_ptr(), fr.data_ptr(),
                                                                   hf.data_ptr(), hs.data_ptr(), best.data_ptr(), bf.data_ptr(),
                                                                   st.data_ptr(), stream),
        "threshold_py": lambda: thr.step_records(probs, frames=fr),
        "ctc": lambda: lib.wekws_hip_ctc_kws_step(h, soft.data_ptr(), args.streams, T, ids.data_ptr(), fr.data_ptr(), res.data_ptr(), stream),
    }
    med, p10, p90 = timed(variants, args.rounds, args.group)
    print(json.dumps(dict(kind="detector_step", streams=args.streams, frames=T, keywords=K, rounds=args.rounds, group=args.group, ms=med,
                          p10=p10, p90=p90, device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--group", type=int, default=4)
    ap.add_argument("--fbank-only", action="store_true")
    ap.add_argument("--root", default=ROOT, help="the checkout whose wekws_amd package is measured")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    assert torch.cuda.is_available(), "bench_stream_mfcc.py measures on the GPU only"
    import wekws_amd
    assert os.path.abspath(os.path.dirname(os.path.dirname(wekws_amd.__file__))) == root, wekws_amd.__file__
    measure_push(args, root)
    if not args.fbank_only:
        measure_detector(args)


if __name__ == "__main__":
    main()
