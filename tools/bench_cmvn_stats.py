#!/usr/bin/env python3
"""Measurements of the global CMVN statistics (wekws_amd.cmvn), one JSON line each; not the bench.py contract.  GPU only.

    python tools/bench_cmvn_stats.py --out profiles/cmvn_stats.jsonl

At (B, 98, 80) for B = 1024 and 8192, with mixed lengths on the device: one CmvnStats.update; Fbank -> update from one-second
PCM; for comparison what torch can do with the same tensors in the same process, (feats.double() * mask).sum((0, 1)) plus the
same of the squares; and on the host the reference's float32 accumulation (tests/cmvn_stats_ref.py::reference_float32, one
thread).  The device rows alternate within one run (update, torch, update, torch, ...) and report the median of the rounds.
Times are device events around groups of back-to-back calls behind a warm-up, as in tools/bench_augment.py; `bytes` is what the
stage must read by its definition -- the valid and padded features once, B T D 4 -- and `hbm_fraction` that over 8 TB/s over
the measured time.  Before anything is timed the update is held to the exact oracle's bar on a slice, and against torch's
double sums on the full tensor."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import cmvn_stats_ref as ref  # noqa: E402
from tools.bench_augment import timeit  # noqa: E402
from wekws_amd.cmvn import CmvnStats  # noqa: E402
from wekws_amd.frontend import Fbank  # noqa: E402

HBM = 8.0e12


def row(out, **kw):
    if "ms" in kw and "bytes" in kw:
        kw["gb_per_s"] = round(kw["bytes"] / kw["ms"] / 1e6, 1)
        kw["hbm_fraction"] = round(kw["bytes"] / HBM * 1e3 / kw["ms"], 3)
    out.append(kw)
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="", help="also write the rows to this file")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the device variants")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_cmvn_stats.py measures on the GPU only"
    out = []
    T, D = 98, 80
    for B in (1024, 8192):
        g = torch.Generator().manual_seed(B)
        feats = (10.0 + 4.0 * torch.randn((B, T, D), generator=g)).cuda()
        lengths = torch.randint(T // 2, T + 1, (B,), generator=g).to(torch.int32)
        lens_d = lengths.cuda()
        mask = (torch.arange(T)[None, :] < lengths[:, None]).to(torch.float64)[:, :, None].cuda()
        st = CmvnStats(D)
        nbytes = B * T * D * 4

        def torch_sums():
            x = feats.double() * mask
            return x.sum((0, 1)), (x * x).sum((0, 1))

        # what is timed computes what it should: the oracle's bar on 64 rows, torch's double sums on all of them
        st.update(feats[:64].contiguous(), lens_d[:64].contiguous())
        want = ref.oracle(ref.valid_rows(feats[:64].cpu().numpy(), lengths[:64].tolist()))
        um, uv, n_ok, cls = ref.inside(st.result(), want)
        assert um <= 1.0 and uv <= 1.0 and n_ok and cls, (um, uv)
        st.reset()
        st.update(feats, lens_d)
        got, (tm, tv) = st.result(), torch_sums()
        rel = max(float((torch.tensor(got["mean_stat"], dtype=torch.float64) - tm.cpu()).abs().max() / tm.abs().max()),
                  float((torch.tensor(got["var_stat"], dtype=torch.float64) - tv.cpu()).abs().max() / tv.abs().max()))
        assert rel < 1e-12 and got["frame_num"] == int(lengths.sum()), rel
        row(out, kind="check", B=B, T=T, D=D, oracle_units_64_rows=[round(um, 4), round(uv, 4)], rel_diff_to_torch_double=rel,
            frame_num=got["frame_num"])
        upd, tor = [], []
        for _ in range(args.rounds):
            upd.append(timeit(lambda: st.update(feats, lens_d)))
            tor.append(timeit(torch_sums))
        for kind, ts in (("update", upd), ("torch (feats.double() * mask).sum((0, 1)) and of the squares", tor)):
            med = sorted(t[0] for t in ts)[len(ts) // 2]
            row(out, kind=kind, B=B, T=T, D=D, ms=round(med, 4), rounds=[round(t[0], 4) for t in ts], p10=round(min(t[1] for t in ts), 4),
                p90=round(max(t[2] for t in ts), 4), bytes=nbytes, utt_per_s=round(B / med * 1e3))
        pcm = (torch.rand((B, 16000), generator=g) * 2 - 1).cuda() * 32768.0
        fb = Fbank(D, window="povey")
        assert tuple(fb(pcm).shape) == (B, T, D)
        med, p10, p90 = timeit(lambda: fb(pcm))
        row(out, kind="fbank80", B=B, samples=16000, ms=round(med, 4), p10=round(p10, 4), p90=round(p90, 4))
        med, p10, p90 = timeit(lambda: st.update(fb(pcm), lens_d))
        row(out, kind="fbank80 -> update", B=B, samples=16000, ms=round(med, 4), p10=round(p10, 4), p90=round(p90, 4), utt_per_s=round(B / med * 1e3))
        # the host path this replaces: the reference's float32 accumulation on one thread (the features already computed)
        torch.set_num_threads(1)
        host, hl = feats.cpu().numpy(), lengths.tolist()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref.reference_float32(host, hl)
            ts.append(time.perf_counter() - t0)
        row(out, kind="host: the reference's float32 accumulation, one thread", B=B, T=T, D=D, ms=round(float(np.median(ts)) * 1e3, 3),
            bytes=nbytes)
        del st, feats, pcm, mask
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
