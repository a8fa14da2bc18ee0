#!/usr/bin/env python3
"""Measurements of wire encodings in the rate bank's fetch (wekws_hip_resample_bank_push_wire), one JSON line per chunk size; not
the bench.py contract.  GPU only.

    python tools/bench_wire.py --out profiles/wire.jsonl

4096 streams of 8 kHz telephony, one 20 ms chunk (160 samples) per stream and push, to 16 kHz int16.  On ONE handle whose streams
are half mu-law, half int16 members of the same rate, in one run:
  mulaw    the mu-law push: (4096, 160) bytes on the device, decoded in the fetch
  int16    the int16 push of the same samples, already decoded, on the device: (4096, 160) int16
  host     what a caller does without wire members: audioop.ulaw2lin per stream on the host, the rows stacked, one upload, the
           int16 push -- timed by the host clock around work that ends in a device synchronise
The two pushes alternate in groups between device events (ms_dev) and are also timed like `host` (ms_wall: one push and a
synchronise, the chunk already on the device).  Every figure is the median and the minimum over the repetitions.  A push of 20 ms
chunks is microseconds of kernel behind tens of microseconds of host call, so ms_dev of that record is the rate at which the host
can queue pushes; a second record repeats the three with 0.3 s chunks (2400 samples), where the kernel is what is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wekws_amd import _capi  # noqa: E402
from wekws_amd.frontend import StreamingResamplerBank  # noqa: E402

B = 4096


def host_decoder():
    """bytes -> int16 bytes of one stream's chunk, and its name"""
    try:
        import audioop
        return (lambda c: audioop.ulaw2lin(c, 2)), "audioop.ulaw2lin"
    except ImportError:                                     # (Python 3.13 dropped audioop: the library's own host decoder)
        lib = _capi.load()

        def decode(c):
            out = np.empty(len(c), dtype=np.int16)
            _capi.check(lib.wekws_hip_wire_decode(1, c, len(c), out.ctypes.data), "wekws_hip_wire_decode")
            return out.tobytes()
        return decode, "wekws_hip_wire_decode"


def device_times(fa, fb, reps, group):
    """ms per call of fa and of fb: alternating groups of calls between device events, behind a warm-up"""
    t_pre = time.perf_counter()                             # an idle MI355X runs its first ~0.25 s of work at lower clocks
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
    return ts


def wall_times(fns, reps):
    """ms per call of every fn, host clock, each call ended by a device synchronise; the fns alternate"""
    ts = [[] for _ in fns]
    for _ in range(2):
        for fn in fns:
            fn()
            torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return ts


def stats(t):
    return dict(median=round(float(np.median(t)), 4), min=round(float(np.min(t)), 4), max=round(float(np.max(t)), 4))


def measure(N, config, args):
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 256, (B, N)).astype(np.uint8)
    decode, decoder_name = host_decoder()
    chunks = [codes[b].tobytes() for b in range(B)]         # as they arrive: one RTP payload per stream
    pcm = np.stack([np.frombuffer(decode(c), dtype=np.int16) for c in chunks])
    rs = StreamingResamplerBank(2 * B, [(8000, "mulaw"), (8000, "s16")], 16000, max_chunk=N)
    ids_mu, ids_16 = np.arange(B), np.arange(B, 2 * B)
    rs.set_rate(ids_16, 8000)
    d_codes, d_pcm = torch.from_numpy(codes).to("cuda"), torch.from_numpy(pcm).to("cuda")
    cap = rs.max_out(N)
    ns = np.full(B, N, dtype=np.int32)

    def push_mulaw():
        return rs.push(d_codes, samples=ns, streams=ids_mu, capacity=cap)

    def push_int16():
        return rs.push(d_pcm, samples=ns, streams=ids_16, capacity=cap)

    def push_host():
        host = np.stack([np.frombuffer(decode(c), dtype=np.int16) for c in chunks])
        return rs.push(torch.from_numpy(host).to("cuda"), samples=ns, streams=ids_16, capacity=cap)

    for _ in range(3):                                      # steady state: every stream holds its history; same bits on both sides
        ya, ca = push_mulaw()
        yb, cb = push_int16()
        assert ca == cb and torch.equal(ya, yb)
    dev = device_times(push_mulaw, push_int16, args.reps, args.group)
    wall = wall_times((push_mulaw, push_int16, push_host), args.reps)
    row = dict(kind="wire", config=config, B=B, chunk=N,
               capacity=cap, samples_per_push=int(ca[0]), reps=args.reps, group=args.group, host_decoder=decoder_name,
               bytes_in=dict(mulaw=B * N, int16=2 * B * N),
               ms_dev=dict(mulaw=stats(dev[0]), int16=stats(dev[1])),
               ms_wall=dict(mulaw=stats(wall[0]), int16=stats(wall[1]), host_decode_upload_int16=stats(wall[2])))
    row["mulaw_over_int16_dev"] = round(row["ms_dev"]["mulaw"]["median"] / row["ms_dev"]["int16"]["median"], 3)
    row["mulaw_within_int16_spread_dev"] = bool(row["ms_dev"]["mulaw"]["median"] <= row["ms_dev"]["int16"]["max"])
    row["host_over_mulaw_wall"] = round(row["ms_wall"]["host_decode_upload_int16"]["median"] / row["ms_wall"]["mulaw"]["median"], 2)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--group", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_wire.py measures on the GPU; none is visible")
    if args.reps < 5:
        sys.exit("at least five repetitions")
    rows = [measure(160, "4096 streams x 160 samples (20 ms at 8 kHz) -> 16 kHz int16, one handle, one run", args),
            measure(2400, "4096 streams x 2400 samples (0.3 s at 8 kHz) -> 16 kHz int16, one handle, one run", args)]
    if args.out:
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
