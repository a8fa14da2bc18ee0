#!/usr/bin/env python3
"""Times one decode step of the CTC spotter -- 4096 streams x 10 frames x 2599 tokens, beams 3 / 20 -- with and without
per-stream keyword sets, on one GPU.  Three cases, alternated round by round in one process:

    a  a baseline build of the library (--baseline-lib: e.g. the parent commit's libwekws_hip.so), every stream in its one set
    b  this tree's library, every stream in set 0
    c  this tree's library, 64 registered sets assigned round-robin (each holds the keywords of set 0, at its own place
       in the tables: the same search, a different record, mask and keyword block per stream)

    timeout -k 10 600 python tools/bench_ctc_kws_sets.py [--baseline-lib PATH] [--out records.json]

Every case decodes the same chunk from the same fresh state, so after each round the result records of all cases must be
byte-identical; the tool fails if they are not.  Prints one JSON record per case: the median over all timed windows of the time
per step, and the lowest / highest of the rounds' medians (the spread between repeats of the same code)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wekws_amd import _capi  # noqa: E402

KWS = [(3, 4, 5), (3, 6, 7)]
V, STREAMS, FRAMES, NSETS = 2599, 4096, 10, 64


def peaky(g, B, T, vocab):
    x = torch.randn(B, T, vocab, generator=g)
    dom = torch.randint(0, 8, (B, T), generator=g) * (torch.rand(B, T, generator=g) < .35)
    x.scatter_add_(2, dom.unsqueeze(2), torch.full((B, T, 1), 7.0))
    return x.softmax(2)


def typed(path):
    lib = C.CDLL(path)
    lib.wekws_hip_ctc_kws_create.restype = C.c_int
    lib.wekws_hip_ctc_kws_create.argtypes = [C.POINTER(_capi.CtcKwsDesc), C.POINTER(C.c_void_p)]
    lib.wekws_hip_ctc_kws_destroy.restype = None
    lib.wekws_hip_ctc_kws_destroy.argtypes = [C.c_void_p]
    lib.wekws_hip_ctc_kws_step.restype = C.c_int
    lib.wekws_hip_ctc_kws_step.argtypes = [C.c_void_p] * 2 + [C.c_int] * 2 + [C.c_void_p] * 4
    lib.wekws_hip_last_error.restype = C.c_char_p
    return lib


class Case:
    def __init__(self, name, lib, nsets):
        self.name, self.lib, self.times, self.rounds = name, lib, [], []
        flat = np.array([t for k in KWS for t in k], np.int32)
        offs = np.array([0] + list(np.cumsum([len(k) for k in KWS])), np.int32)
        ts = np.array(sorted({0} | {t for k in KWS for t in k}), np.int32)
        d = _capi.CtcKwsDesc(vocab=V, score_beam=3, path_beam=20, num_keywords=len(KWS), keyword_tokens=flat.ctypes.data,
                             keyword_offsets=offs.ctypes.data, token_set=ts.ctypes.data, token_set_len=len(ts), min_frames=5,
                             max_frames=250, interval_frames=50, downsampling=1, max_streams=STREAMS, prefix_capacity=564,
                             device=0, threshold=0.5)
        self.h = C.c_void_p()
        self.ok(lib.wekws_hip_ctc_kws_create(C.byref(d), C.byref(self.h)), "create")
        if nsets:
            lib.wekws_hip_ctc_kws_add_set.restype = C.c_int
            lib.wekws_hip_ctc_kws_add_set.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_int32),
                                                      C.c_void_p]
            lib.wekws_hip_ctc_kws_assign.restype = C.c_int
            lib.wekws_hip_ctc_kws_assign.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
            ids = []
            for _ in range(nsets):
                out = C.c_int32(-1)
                self.ok(lib.wekws_hip_ctc_kws_add_set(self.h, flat.ctypes.data, offs.ctypes.data, len(KWS), ts.ctypes.data, len(ts),
                                                      0.5, C.byref(out), None), "add_set")
                ids.append(out.value)
            streams = np.arange(STREAMS, dtype=np.int32)
            sets = np.array([ids[s % nsets] for s in range(STREAMS)], np.int32)
            self.ok(lib.wekws_hip_ctc_kws_assign(self.h, streams.ctypes.data, sets.ctypes.data, STREAMS, None), "assign")
        self.res = torch.empty((STREAMS, 32), dtype=torch.uint8, device="cuda")

    def ok(self, rc, what):
        if rc != 0:
            raise SystemExit(f"{self.name}: {what} failed ({rc}): {self.lib.wekws_hip_last_error().decode()}")

    def step(self, chunk, ids):
        s = torch.cuda.current_stream().cuda_stream
        self.ok(self.lib.wekws_hip_ctc_kws_step(self.h, chunk.data_ptr(), STREAMS, FRAMES, ids.data_ptr(), None,
                                                self.res.data_ptr(), C.c_void_p(s)), "step")

    def run(self, chunk, ids, windows, steps, keep):
        """`windows` timed windows of `steps` back-to-back steps each; the times are per step"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(windows):
            e0.record()
            for _ in range(steps):
                self.step(chunk, ids)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / steps)
        if keep:
            self.times += ts
            self.rounds.append(float(np.median(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", help="a library built from the commit to compare against (case a)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--windows", type=int, default=4, help="timed windows per case and round")
    ap.add_argument("--steps", type=int, default=1000, help="steps per window (a window of about a quarter of a second)")
    ap.add_argument("--out", help="also write the records to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctc_kws_sets: no GPU (there is no CPU fallback, and a CPU time would say nothing)")
    g = torch.Generator().manual_seed(1)
    chunk = peaky(g, STREAMS, FRAMES, V).cuda().contiguous()
    ids = torch.arange(STREAMS, dtype=torch.int32, device="cuda")
    here = typed(_capi.lib_path())
    cases = []
    if args.baseline_lib:
        cases.append(Case("a_baseline", typed(args.baseline_lib), 0))
    cases += [Case("b_set0", here, 0), Case("c_64_sets", here, NSETS)]
    for r in range(args.rounds + 1):                 # round 0 warms every case up and is not kept
        for c in cases:
            c.run(chunk, ids, args.windows if r else 1, args.steps, keep=r > 0)
        ref = cases[0].res.cpu().numpy().tobytes()
        for c in cases[1:]:
            if c.res.cpu().numpy().tobytes() != ref:
                raise SystemExit(f"round {r}: the records of {c.name} differ from those of {cases[0].name}")
    out = []
    for c in cases:
        out.append(dict(case=c.name, streams=STREAMS, frames=FRAMES, V=V, windows=len(c.times), steps_per_window=args.steps, median_ms=float(np.median(c.times)),
                        round_median_min_ms=min(c.rounds), round_median_max_ms=max(c.rounds),
                        p10_ms=float(np.percentile(c.times, 10)), p90_ms=float(np.percentile(c.times, 90))))
        c.lib.wekws_hip_ctc_kws_destroy(c.h)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for r in out:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
