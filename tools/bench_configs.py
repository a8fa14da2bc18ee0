#!/usr/bin/env python3
"""Secondary measurements for the other BASELINE.json configs (one JSON line each, not the bench.py contract):
batch throughput of every backbone, streaming per-frame latency (B=1, 10-frame chunks, carried cache), fbank
front-end throughput.  GPU only.   python tools/bench_configs.py > gpurun_out/configs.jsonl"""
# (also: the streaming front end, filter `stream_frontend`; the streaming resampler in front of it, filter `resample`)
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wekws_amd import pack  # noqa: E402
from wekws_amd.frontend import Fbank  # noqa: E402
from wekws_amd.model.kws_model import init_model  # noqa: E402
from wekws_amd.utils import synth  # noqa: E402


def build(name):
    cfg = dict(synth.MODEL_CONFIGS[name])
    m = init_model(cfg)
    sd = synth.synth_state_dict(pack.model_spec(cfg), 1234)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return cfg, m.cuda().eval().freeze()      # weights are final: skip the per-call version check


def timeit(fn, warm=5, reps=30, group=10):
    """Throughput timing: `group` back-to-back launches between two events (the stream never drains, so host launch
    overhead is hidden as in bench.py), repeated `reps` times; returns median / p10 / p90 of the per-launch time."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t_pre = time.perf_counter()       # an idle MI355X runs its first ~0.25 s of work at lower clocks: measure behind that
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


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else ""   # optional substring filter on the model name
    out = []
    # FSMN-CTC: 400-d spliced features at frame_skip 3 (fsmn_ctc.yaml:21-25): 98 fbank frames (1 s) -> T = 32; 2 s -> 64
    for name, B, T in (("fsmn_ctc", 1024, 32), ("fsmn_ctc", 1024, 64), ("fsmn_ctc", 4096, 32)):
        if only not in name:
            continue
        cfg, m = build(name)
        x = torch.from_numpy(synth.synth_feats(B, T, cfg["input_dim"], seed=1)).cuda()
        med, p10, p90 = timeit(lambda: m(x), reps=6, group=6)
        out.append(dict(kind="batch", model=name, B=B, T=T, ms=round(med, 4), p10=round(p10, 4), p90=round(p90, 4),
                        utts_per_s=round(B / med * 1e3, 1), frames_per_s=round(B * T / med * 1e3, 1)))
        print(json.dumps(out[-1]), flush=True)
    # "@f16": WEKWS_HIP_PRECISION_F16, the reduced-precision mode of BASELINE.json config 5 (fp16 weights + fp16 MFMA
    # pointwise conv; MDTC + 12-class GlobalClassifier, 1024 utterances per GPU of the 8192)
    for name, B in (("ds_tcn_h256", 1024), ("ds_tcn_h256", 8192), ("mdtc_h64", 1024), ("mdtc_h64", 8192),
                    ("mdtc_h64_global12", 1024), ("mdtc_h64_global12@f16", 1024), ("mdtc_h64_global12@f16", 8192),
                    ("mdtc_h64@f16", 1024), ("ds_tcn_h256@f16", 1024),
                    ("mdtc_small", 1024), ("ds_tcn_h64", 1024), ("tcn_h64", 1024),
                    ("gru_2x128", 256), ("gru_2x128", 1024), ("gru_2x128", 16384)):
        if only not in name:
            continue
        cfg, m = build(name.split("@")[0])
        if "@" in name:
            m.set_precision(name.split("@")[1]).freeze()
        x = torch.from_numpy(synth.synth_feats(B, 98, cfg["input_dim"], seed=1)).cuda()
        med, p10, p90 = timeit(lambda: m(x), reps=10 if B <= 1024 else 4, group=10 if B <= 1024 else 4)
        out.append(dict(kind="batch", model=name, B=B, T=98, ms=round(med, 4), p10=round(p10, 4), p90=round(p90, 4),
                        utts_per_s=round(B / med * 1e3, 1)))
        print(json.dumps(out[-1]), flush=True)
    # streaming latency: B streams, 10-frame chunks, cache carried, host-timed per chunk (includes launch overhead)
    for name, B in (("gru_2x128", 1), ("gru_2x128", 256), ("ds_tcn_h256", 1), ("ds_tcn_h256", 256), ("mdtc_h64", 1),
                    ("mdtc_h64", 256), ("fsmn_ctc", 1), ("fsmn_ctc", 256)):
        if only not in name:
            continue
        cfg, m = build(name)
        x = torch.from_numpy(synth.synth_feats(B, 10, cfg["input_dim"], seed=2)).cuda()
        _, cache = m(x)
        t_pre = time.perf_counter()   # (steady clocks, as in timeit)
        while time.perf_counter() - t_pre < 0.3:
            for _ in range(20):
                _, cache = m(x, cache)
            torch.cuda.synchronize()
        n = 200
        t0 = time.perf_counter()
        for _ in range(n):
            y, cache = m(x, cache)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / n * 1e3
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            y, cache = m(x, cache)
        b.record()
        torch.cuda.synchronize()
        dev = a.elapsed_time(b) / n
        out.append(dict(kind="stream", model=name, B=B, chunk=10, ms_per_chunk_wall=round(wall, 4),
                        ms_per_chunk_stream=round(dev, 4), us_per_frame=round(dev * 100, 2)))
        print(json.dumps(out[-1]), flush=True)
    # streaming THROUGHPUT with many concurrent streams (10-frame chunks, caches carried): stream-chunks per second;
    # lds_cache = the streaming kernel that keeps each stream's cache in LDS (ds256_stream.hip.h, the default for
    # chunks of <= 16 frames); False = option stream = 0, the batch kernel fed the same chunks
    if only in "manystreams":
        for mname, B in [("ds_tcn_h256", b) for b in (1, 256, 1024, 4096, 16384)] + [("mdtc_h64", b) for b in (1, 256, 4096)]:
            for packed in (True, False):
                cfg, m = build(mname)
                m.set_option("stream", 1 if packed else 0).freeze()
                x = torch.from_numpy(synth.synth_feats(B, 10, 40, seed=2)).cuda()
                _, cache = m(x)
                state = {"c": cache}

                def step():
                    _, state["c"] = m(x, state["c"])
                med, p10, p90 = timeit(step, reps=6, group=6)
                out.append(dict(kind="manystreams", model=mname, B=B, chunk=10, lds_cache=packed, ms=round(med, 4),
                                chunks_per_s=round(B / med * 1e3, 1), frames_per_s=round(B * 10 / med * 1e3, 1)))
                print(json.dumps(out[-1]), flush=True)
    # end-to-end on the device, PCM resident in HBM: (a) fbank40 -> DS-TCN h256 posteriors; (b) fbank80 -> context
    # expansion(2, 2) / skip 3 -> FSMN-CTC logits -> fused softmax + top-3 (what stream_kws_ctc.py's decoder consumes)
    if only in "e2e":
        from wekws_amd import ctc
        from wekws_amd.frontend import splice_skip
        B = 1024
        pcm = torch.from_numpy(synth.synth_pcm(B, 16000, seed=3)).cuda()
        _, m1 = build("ds_tcn_h256")
        fb40 = Fbank(40)
        med, p10, p90 = timeit(lambda: m1(fb40(pcm)), reps=6, group=6)
        out.append(dict(kind="e2e", pipeline="pcm -> fbank40 -> ds_tcn_h256 -> posteriors", B=B, ms=round(med, 4),
                        utts_per_s=round(B / med * 1e3, 1)))
        print(json.dumps(out[-1]), flush=True)
        _, m2 = build("fsmn_ctc")
        fb80 = Fbank(80)
        med, p10, p90 = timeit(lambda: ctc.softmax_topk(m2(splice_skip(fb80(pcm), 2, 2, 3))[0], 3), reps=6, group=6)
        out.append(dict(kind="e2e", pipeline="pcm -> fbank80 -> splice(2,2)/skip3 -> fsmn_ctc -> softmax+top3", B=B,
                        ms=round(med, 4), utts_per_s=round(B / med * 1e3, 1)))
        print(json.dumps(out[-1]), flush=True)
    # host buffers in, host scores out (what a caller without device residency pays): pinned feats -> H2D -> DS-TCN h256
    # -> D2H of the posteriors.  "serial": one stream.  "overlapped": copies on their own streams, 3 batches in flight.
    if only in "pcie":
        B, T = 1024, 98
        _, m = build("ds_tcn_h256")
        nbuf = 3
        hx = [torch.from_numpy(synth.synth_feats(B, T, 40, seed=i)).pin_memory() for i in range(nbuf)]
        hy = [torch.empty(B, T, 2).pin_memory() for _ in range(nbuf)]
        dx = [torch.empty(B, T, 40, device="cuda") for _ in range(nbuf)]
        dy = [None] * nbuf

        def serial(n):
            for i in range(n):
                j = i % nbuf
                dx[j].copy_(hx[j], non_blocking=True)
                y, _ = m(dx[j])
                hy[j].copy_(y, non_blocking=True)

        up, comp, down = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
        ev_up = [torch.cuda.Event() for _ in range(nbuf)]
        ev_c = [torch.cuda.Event() for _ in range(nbuf)]
        ev_d = [torch.cuda.Event() for _ in range(nbuf)]

        def overlapped(n):
            for i in range(n):
                j = i % nbuf
                with torch.cuda.stream(up):
                    up.wait_event(ev_c[j])                      # the previous forward on this buffer has read it
                    dx[j].copy_(hx[j], non_blocking=True)
                    ev_up[j].record(up)
                with torch.cuda.stream(comp):
                    comp.wait_event(ev_up[j])
                    comp.wait_event(ev_d[j])                    # its previous scores have left the device
                    dy[j], _ = m(dx[j])
                    ev_c[j].record(comp)
                with torch.cuda.stream(down):
                    down.wait_event(ev_c[j])
                    hy[j].copy_(dy[j], non_blocking=True)
                    ev_d[j].record(down)

        for label, fn in (("serial", serial), ("overlapped", overlapped)):
            fn(6)
            torch.cuda.synchronize()
            n = 60
            t0 = time.perf_counter()
            fn(n)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / n * 1e3
            out.append(dict(kind="pcie", mode=label, model="ds_tcn_h256", B=B, ms=round(ms, 4),
                            utts_per_s=round(B / ms * 1e3, 1), h2d_GBs=round(B * T * 40 * 4 / ms / 1e6, 1)))
            print(json.dumps(out[-1]), flush=True)
    # streaming front end: 4096 streams in steady state, 4800-sample chunks (30 frames per push) -- time per push of the front end
    # alone, of PCM -> detection (front end -> fsmn_ctc300 with carried caches -> CTC decoder), and in the same run the one-shot
    # Fbank + splice_skip on the same rows x frames held as whole signals (30 frames = 5040 samples)
    if only in "stream_frontend":
        from wekws_amd.frontend import StreamingFrontEnd, splice_skip
        from wekws_amd.stream import BatchedKeyWordSpotter
        B, n = 4096, 4800
        g = torch.Generator(device="cuda").manual_seed(7)
        chunk = torch.randint(-20000, 20000, (B, n), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
        whole = torch.randint(-20000, 20000, (B, 400 + 29 * 160), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
        for label, bins, window, left, right, skip in (("80/povey/(2,2)/skip3", 80, "povey", 2, 2, 3),
                                                       ("40/hamming/no context", 40, "hamming", 0, 0, 1)):
            fe = StreamingFrontEnd(B, bins, window, left, right, skip, max_chunk=n)
            buf = torch.zeros((B, fe.max_frames(n), fe.feat_dim), device="cuda")
            frames = fe.push(chunk, out=buf)[1]
            frames = fe.push(chunk, out=buf)[1]                     # steady state: every stream holds its leftover and frames
            med, p10, p90 = timeit(lambda: fe.push(chunk, out=buf), reps=10, group=10)
            fb1 = Fbank(bins, window=window)
            one = (lambda: splice_skip(fb1(whole), left, right, skip)) if (left or skip > 1) else (lambda: fb1(whole))
            omed, op10, op90 = timeit(one, reps=10, group=10)
            row = dict(kind="stream_frontend", config=label, B=B, chunk=n, frames_per_push=int(frames[0]), ms_push=round(med, 4),
                       p10=round(p10, 4), p90=round(p90, 4), ms_oneshot_same_frames=round(omed, 4), oneshot_p10=round(op10, 4),
                       oneshot_p90=round(op90, 4), push_over_oneshot=round(med / omed, 3),
                       chunks_per_s=round(B / med * 1e3, 1))
            if left:
                _, m = build("fsmn_ctc300")
                kws = BatchedKeyWordSpotter(m, {"k0": (1, 2, 3)}, 0.5, B, num_bins=bins, window=window, left=left, right=right,
                                            skip=skip, max_chunk=n)
                kws.forward(chunk)
                dmed, dp10, dp90 = timeit(lambda: kws.forward(chunk), warm=2, reps=5, group=4)
                row.update(ms_pcm_to_detection=round(dmed, 4), detection_p10=round(dp10, 4), detection_p90=round(dp90, 4),
                           model="fsmn_ctc300")
            out.append(row)
            print(json.dumps(out[-1]), flush=True)
    # streaming resampler: 4096 streams x 14400-sample chunks at 48 kHz (0.3 s) in steady state -- time per push, the same as a
    # fraction of the time to move the call's input and output bytes at the 8 TB/s of DESIGN.md section 5, and in the same run PCM
    # -> detection (fsmn_ctc300) from 16 kHz chunks and from the 48 kHz chunks of the same duration
    if only in "resample":
        from wekws_amd.frontend import StreamingResampler
        from wekws_amd.stream import BatchedKeyWordSpotter
        B, n = 4096, 14400
        g = torch.Generator(device="cuda").manual_seed(7)
        chunk = torch.randint(-20000, 20000, (B, n), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
        for dt in (torch.int16, torch.float32):
            rs = StreamingResampler(B, 48000, 16000, max_chunk=n, out_dtype=dt)
            cap = rs.max_out(n)
            counts = rs.push(chunk, capacity=cap)[1]
            counts = rs.push(chunk, capacity=cap)[1]                # steady state: every stream holds its history
            med, p10, p90 = timeit(lambda: rs.push(chunk, capacity=cap), reps=10, group=10)
            moved = B * (n * 2 + cap * (2 if dt == torch.int16 else 4))
            row = dict(kind="resample", config="48000->16000/" + ("int16" if dt == torch.int16 else "float32") + " out", B=B, chunk=n,
                       samples_per_push=int(counts[0]), ms_push=round(med, 4), p10=round(p10, 4), p90=round(p90, 4),
                       bytes_moved=moved, ms_at_8TBs=round(moved / 8e12 * 1e3, 4), hbm_fraction=round(moved / 8e12 * 1e3 / med, 3),
                       chunks_per_s=round(B / med * 1e3, 1))
            if dt == torch.int16:
                _, m = build("fsmn_ctc300")
                fe_kw = dict(num_bins=80, window="povey", left=2, right=2, skip=3)
                for label, rate, c in (("ms_pcm_to_detection_16k", None, chunk[:, :n // 3].contiguous()), ("ms_pcm_to_detection_48k", 48000, chunk)):
                    extra = {} if rate is None else dict(input_sample_rate=rate)
                    kws = BatchedKeyWordSpotter(m, {"k0": (1, 2, 3)}, 0.5, B, max_chunk=int(c.size(1)), **fe_kw, **extra)
                    kws.forward(c)
                    dmed, dp10, dp90 = timeit(lambda: kws.forward(c), warm=2, reps=5, group=4)
                    row.update({label: round(dmed, 4), label + "_p10": round(dp10, 4), label + "_p90": round(dp90, 4)})
                    del kws
                row.update(model="fsmn_ctc300")
            out.append(row)
            print(json.dumps(out[-1]), flush=True)
    fb = Fbank(40)
    for B in ((1024, 8192) if only in "fbank" else ()):
        pcm = torch.from_numpy(synth.synth_pcm(B, 16000, seed=3)).cuda()
        med, p10, p90 = timeit(lambda: fb(pcm))
        out.append(dict(kind="fbank", B=B, nsamp=16000, ms=round(med, 4), utts_per_s=round(B / med * 1e3, 1),
                        GBs=round((B * 16000 * 4 + B * 98 * 40 * 4) / med / 1e6, 1)))
        print(json.dumps(out[-1]), flush=True)


if __name__ == "__main__":
    main()
