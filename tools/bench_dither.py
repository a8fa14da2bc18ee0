#!/usr/bin/env python3
"""Measurements of the dithered fbank front end (wekws_amd.frontend.Fbank(dither=...)), one JSON line each; not the bench.py
contract.  GPU only.

    python tools/bench_dither.py --out profiles/dither.jsonl

At B = 1024 and 8192 one-second rows, 40 bins (Hamming) and 80 bins (Povey), float32 and int16 PCM, three variants that alternate
within one run (dithered, plain, torch, dithered, ...) and report the median of the rounds:
  dithered  Fbank(dither=1.0): the noise is drawn in the kernel's fetch (csrc/philox.hip.h)
  plain     Fbank() on the same PCM: the kernel the ratio `dithered / plain` of each row is measured against
  torch     what a user could do without the feature: randn(B, frames, 400), unfold the PCM into frames, add, then a plain fbank of
            the (B * frames, 400) frames as utterances with shift = length
Times are device events around groups of back-to-back calls behind a warm-up (tools/bench_augment.py::timeit).  Before anything is
timed the dithered features of a few rows are held to the float64 frame oracle (tests/dither_ref.py) at the suite's bar."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dither_ref as dr  # noqa: E402
from tests.helpers import K_FBANK  # noqa: E402
from tools.bench_augment import timeit  # noqa: E402
from wekws_amd.frontend import Fbank  # noqa: E402

FL, SHIFT, NSAMP = 400, 160, 16000


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="", help="also write the rows to this file")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the variants")
    ap.add_argument("--batches", type=int, nargs="*", default=[1024, 8192])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_dither.py measures on the GPU only"
    out = []

    def row(**kw):
        out.append(kw)
        print(json.dumps(kw), flush=True)

    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        base = torch.round(torch.randn((B, NSAMP), generator=g) * 3000.0).clamp_(-32767, 32767)
        for bins, window in ((40, "hamming"), (80, "povey")):
            for dtype in ("f32", "i16"):
                pcm = base.cuda() if dtype == "f32" else base.to(torch.int16).cuda()
                fd, fp = Fbank(bins, window=window, dither=1.0, seed=dr.SEED), Fbank(bins, window=window)
                fframes = Fbank(bins, frame_length=FL, frame_shift=FL, window=window)
                nf = fd.num_frames(NSAMP)
                # what is timed computes what it should: four rows against the frame oracle
                got = fd(pcm[:4].contiguous(), first_row=0).cpu().numpy()
                u = max(float(dr.frame_units(got[b], dr.dithered_frames(base[b].numpy(), dr.SEED, b, FL, SHIFT, 1.0), bins, 16000, FL,
                                             int(window == "povey")).max()) for b in range(4))
                assert u <= K_FBANK, u

                def torch_way():
                    z = torch.randn((B, nf, FL), device="cuda")
                    frames = pcm.unfold(1, FL, SHIFT).to(torch.float32) + z
                    return fframes(frames.reshape(B * nf, FL)).view(B, nf, bins)

                assert tuple(torch_way().shape) == tuple(fd(pcm).shape) == (B, nf, bins)
                td, tp, tt = [], [], []
                for _ in range(args.rounds):
                    td.append(timeit(lambda: fd(pcm)))
                    tp.append(timeit(lambda: fp(pcm)))
                    tt.append(timeit(torch_way, reps=10, group=2))
                med = {}
                for kind, ts in (("dithered", td), ("plain", tp), ("torch randn + unfold + add + fbank of frames", tt)):
                    med[kind] = sorted(t[0] for t in ts)[len(ts) // 2]
                    row(kind=kind, B=B, bins=bins, window=window, pcm=dtype, frames=nf, ms=round(med[kind], 4),
                        rounds=[round(t[0], 4) for t in ts], p10=round(min(t[1] for t in ts), 4), p90=round(max(t[2] for t in ts), 4),
                        utt_per_s=round(B / med[kind] * 1e3))
                row(kind="ratio", B=B, bins=bins, window=window, pcm=dtype, oracle_units_4_rows=round(u, 2),
                    dithered_over_plain=round(med["dithered"] / med["plain"], 3),
                    torch_over_dithered=round(med["torch randn + unfold + add + fbank of frames"] / med["dithered"], 2))
                del pcm
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
