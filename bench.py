#!/usr/bin/env python3
"""Headline benchmark: 1-second utterances/s through the fused DS-TCN forward on MI355X, plus the per-frame streaming
latency that is the other half of BASELINE.json's metric.

    python bench.py                                  # 1 GPU, 50 timed steps after 10 warm-up steps
    python bench.py --gpus N --steps K --warmup W    # N > 1 without a launcher: spawns N ranks itself (torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W       # the driver's own launch: one rank per GPU over RCCL
    python bench.py ... --dump-outputs DIR           # also writes the last timed step's outputs to DIR/*.npy (dump_outputs)
    python bench.py ... --full                       # also everything else the benchmark measures (below), ~2 minutes more

A plain run does only what the headline needs: set up, `--preheat`, W warm-up steps, the K timed steps, `--dump-outputs`,
the contract line.  Everything else -- `value_no_preheat`, `step_ms`, `cpu_baseline`, the secondary workloads and the
side file -- is measured only with `--full`; the K timed steps and the fields they give are the same either way.

A "step" is one pass of the hot path (KWSModel.forward: 40-d fbank features -> per-frame posteriors + streaming cache,
what wekws/bin/score.py:125 calls) over one batch of synthetic 1-s utterances already resident in HBM.  Workload
(BASELINE.json metric / SURVEY.md section 8d): DS-TCN h256 (287,490 params, examples/hi_xiaowen/s0/conf/ds_tcn.yaml),
B = 1024 utterances per GPU, T = 98 frames.  Multi-GPU: utterance-parallel, one process per GPU, the weights broadcast
once over RCCL, no collective in the timed forward (weak scaling: 1024 utterances per GPU).

Timing: `--preheat` seconds (default 0.5) of the same forward to bring the GPU out of its idle power state -- an idle
MI355X runs its first ~0.25 s of work at lower clocks: 0.293 ms per step right after 10 steps, 0.244 ms after 1000 --,
then W warm-up steps, then EXACTLY K steps between barrier + torch.cuda.synchronize() on both sides, wall clock, MAX
over ranks -> `value`, `ms_per_step`.  The K steps also sit between two HIP events on the launch stream: that time / K is
the average launch duration the roofline uses (`roofline.kernel_ms`).  `step_ms` (--full) = median / p10 / p90 of >= 50
samples taken right after the timed region, each the mean of 4 back-to-back steps between two HIP events (an event pair
around every single launch adds ~7 us to it and to the job).

Rank 0 prints the contract as ONE compact JSON line, LAST on stdout (< 6 KB: the driver keeps an 8 KB tail): the contract
fields, `config` and `roofline`; with --full also `cpu_baseline`, `value_no_preheat`, `step_ms` and a `summary` of the
secondary workloads.  With --full everything else -- the verbose records below -- goes to a side file (`--extras-out`; the
default is in emit()) and to EARLIER stdout lines of the form `extras <key> = <json>` (which do not start with '{').
  roofline        dominant kernel of `value` (default precision: ds256 register-resident kernel, 3 x fp16 MFMA per MAC on
                  block-floating hi/lo operands, so the peak for ALGORITHMIC flops is 2500 / 3 TF).  `kernel` and `traffic` (HBM
                  bytes per launch from rocprofv3 PMC passes: 2 x FETCH_SIZE + WRITE_SIZE, MI355X_MICROARCH.md's gfx950
                  correction) are reported only when profiles/pmc_traffic.json was taken with the very library file this run
                  loads (sha-256 match) on this workload -- else null.
  value_no_preheat   (--full) the contract's W + K steps taken FIRST, on the idle GPU, before any preheat (`--preheat 0` gives
                  the same as `value`): both readings of "W warm-up steps" exist in one line.
  cpu_baseline    (--full) the reference's CPU path (PyTorch CPU operator sequence, oracle/torch_ref.py) on this box's host cores; the
                  best of: all hardware threads, one core, a thread sweep, one pinned OpenMP thread per physical core, and
                  P processes x 4 pinned threads (utterances split as over GPU ranks); rows in extras `cpu_baseline_detail`.
extras (--full, side file):
  value_single_output_buffer   the same steps with the result dropped at once (one 110 MB cache buffer recycled).
  f32             the same batch with precision F32 (exact-f32 MFMA kernel), roofline against the 157.3 TF f32 matrix peak.
  also / score_only / gru / small_recipes   MDTC h64 (BASELINE config 2's model), posteriors only, GRU 2x128, DS-TCN h64, MDTC small.
  config4_shard / config5   BASELINE.json configs 4 and 5 as ONE GPU sees them: B = 8192 per launch; the 12-class MDTC +
                  GlobalClassifier with precision "f16" (ONE fp16 MFMA per product; roofline = the full 2500 TF).
  latency / latency_chunk80   streaming with the carried cache (stream_kws_ctc.py:482-514, keyword_spotting.cc:56-95): us per
                  frame, median / p10 / p90 over consecutive chunks, at 1 and 256 streams; `cpu` = the CPU port, B = 1.
  rooflines_other ds256_stream_kernel at 4096 streams (HBM-bound: the cache round trip) and fbank_kernel.
  audio_to_posteriors   fbank_kernel + the headline forward back to back on 1024 x 1 s of PCM.
  comm            (N > 1, in the line) backend, world size, bytes and wall time of the ONE weight broadcast; per-rank rates.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_UTT = {"ds_tcn_h256": 55_093_248, "mdtc_h64": 28_888_832, "gru_2x128": 39_588_864,  # SURVEY.md 8d (T = 98)
                "mdtc_small": 5_889_408, "mdtc_h64_global12": 28_873_472,
                "ds_tcn_h64": 2 * 98 * (40 * 64 + 4 * (8 * 64 + 64 * 64) + 64)}                # = 4,126,976 (hey_snips ds_tcn.yaml)
BYTES_PER_UTT = 98 * 40 * 4 + 98 * 2 * 4          # features in + posteriors out = 16,464 B
CACHE_BYTES_PER_UTT = 256 * 105 * 4                # the (256, 105) streaming cache forward() also returns
CACHE_BYTES = {"ds_tcn_h256": 256 * 105 * 4, "mdtc_h64": 64 * 244 * 4, "gru_2x128": 2 * 128 * 4,   # per utterance / stream
               "mdtc_h64_global12": 64 * 244 * 4}
PEAK_F32_TFLOPS = 157.3                            # MI355X_MICROARCH.md: f32 MFMA == f32 vector peak
PEAK_F16_TFLOPS = 2500.0                           # MI355X_MICROARCH.md: dense fp16 / bf16 MFMA peak
PEAK_HBM_GBS = 8000.0
MAX_LINE_BYTES = 6000                              # the driver keeps an 8 KB tail of stdout: the contract line must fit in it


def pct(ts):
    return {"median": round(float(np.median(ts)), 4), "p10": round(float(np.percentile(ts, 10)), 4),
            "p90": round(float(np.percentile(ts, 90)), 4)}


def lib_sha16():
    from wekws_amd import _capi
    try:
        with open(_capi.lib_path(), "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()[:16]
    except Exception:
        return None


def build_model(torch, init_model, pack, synth, name, dev, precision="default", seed=1234):
    cfg = dict(synth.MODEL_CONFIGS[name])
    sd = synth.synth_state_dict(pack.model_spec(cfg), seed)
    m = init_model(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return cfg, sd, m.to(dev).eval().set_precision(precision).freeze()


GROUP = 4   # launches between two HIP events of a step-time sample (an event pair around EVERY launch adds ~7 us to it)


def time_steps(torch, fn, steps, warmup, group=GROUP):
    """`steps` samples of the step time: each the mean of `group` back-to-back launches between two HIP events on the
    current stream (ms)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    if warmup:                                                        # a fresh workload: steady clocks first (--preheat)
        t_pre = time.perf_counter()
        while time.perf_counter() - t_pre < 0.3:
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        for _ in range(group):
            fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) / group for a, b in ev]


def mfma_roofline(model_name, B, kern_ms, precision):
    flop = FLOP_PER_UTT[model_name] * B
    ach = flop / (kern_ms * 1e-3) / 1e12
    if precision == "f32":
        peak, note = PEAK_F32_TFLOPS, "exact-f32 MFMA peak (v_mfma_f32_16x16x4_f32 issues at the vector-f32 rate)"
    elif precision == "f16":
        peak, note = PEAK_F16_TFLOPS, "dense fp16 MFMA peak, one product per MAC"
    else:
        peak, note = PEAK_F16_TFLOPS / 3.0, ("algorithmic flops vs dense fp16 MFMA peak 2500 TF / 3 products per MAC; "
                                             "executed MFMA rate = 3 x achieved")
    hbm = BYTES_PER_UTT * B / (kern_ms * 1e-3) / 1e9
    return {"bound": "mfma", "achieved": round(ach, 3), "peak": round(peak, 1), "unit": "TFLOP/s",
            "frac": round(ach / peak, 4), "peak_note": note, "kernel_ms": round(kern_ms, 4), "flop_per_launch": flop,
            "frac_of_f32_mfma_peak": round(ach / PEAK_F32_TFLOPS, 4),
            "algorithmic_bytes_per_launch": BYTES_PER_UTT * B,
            "algorithmic_bytes_per_launch_with_cache_out": (BYTES_PER_UTT + CACHE_BYTES.get(model_name, 0)) * B,
            "hbm_achieved_GBs": round(hbm, 2), "hbm_peak_GBs": PEAK_HBM_GBS, "hbm_frac": round(hbm / PEAK_HBM_GBS, 6)}


def attach_profile(roof, model_name, B, precision):
    """`kernel` / `traffic` from the committed PMC passes -- only if they were taken on the library file loaded now."""
    try:
        pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        rec = pm.get(f"{model_name}/B{B}/{precision}")
        if rec and pm.get("lib_sha16") and pm["lib_sha16"] == lib_sha16():
            roof["kernel"] = rec["kernel"]
            roof["traffic"] = rec["traffic_bytes_per_launch"]
            roof["traffic_unit"] = ("HBM bytes per launch = 2 x FETCH_SIZE + WRITE_SIZE from separate rocprofv3 --pmc passes: "
                                    "FETCH corrected x2 as MI355X_MICROARCH.md prescribes for gfx950, WRITE as reported "
                                    "(calibrated: exact on three store patterns of known size incl. the cache's 28-byte runs, "
                                    "profiles/r03_write_size_calibration.txt); both count at the L2 - fabric boundary, so traffic "
                                    "the 256 MB memory-side cache absorbs is included (the GRU wavefront's hand-over rings)")
            roof["traffic_source"] = rec.get("profile") or pm.get("profile")
            roof["kernel_avg_ms_rocprof"] = rec.get("kernel_avg_ms")
            return
    except Exception:
        pass
    roof["traffic"] = None
    roof["traffic_note"] = "no PMC profile of this library build under profiles/ (see tools/pmc.sh)"


def compact_roofline(r):
    """The fields of the contract line (the verbose record, with the notes on how the counters are read, goes to the extras)."""
    keep = ("bound", "achieved", "peak", "unit", "frac", "kernel", "kernel_ms", "kernel_avg_ms_rocprof", "traffic",
            "traffic_source", "flop_per_launch", "algorithmic_bytes_per_launch", "algorithmic_bytes_per_launch_with_cache_out",
            "hbm_frac")
    out = {k: r[k] for k in keep if k in r}
    out.setdefault("traffic", None)
    out["peak_note"] = {PEAK_F32_TFLOPS: "f32 MFMA peak", PEAK_F16_TFLOPS: "dense fp16 MFMA peak"}.get(
        r["peak"], "dense fp16 MFMA peak 2500 TF / 3 products per MAC (hi/lo split operands); algorithmic flops")
    return out


def emit(out, extra, extras_out):
    """Rank 0's output: the extras as earlier stdout lines that do NOT start with '{' and as a side file; then, LAST, the one
    compact JSON line of the contract (the driver parses the last line and keeps an 8 KB tail of stdout)."""
    path = extras_out or os.path.join(ROOT, "gpurun_out", "bench_extras.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump({"contract_line": out, "extras": extra}, f, indent=1)
        out["extras_file"] = os.path.relpath(path, ROOT)
    except OSError as e:
        out["extras_file"] = f"not written: {e}"[:120]
    for k, v in extra.items():
        print(f"extras {k} = {json.dumps(v)}")
    print_line(out)


def print_line(out):
    """The one compact JSON line of the contract, LAST on stdout (a plain run prints nothing else)."""
    line = json.dumps(out)
    assert len(line) <= MAX_LINE_BYTES, f"contract line grew to {len(line)} bytes (limit {MAX_LINE_BYTES})"
    sys.stdout.flush()
    print(line, flush=True)


DUMP_BYTES = 64 << 20                              # --dump-outputs: at most this much in all, over every array and rank
NPY_HEADER_BYTES = 4096                            # an upper bound of one .npy file's header (numpy writes 128 .. a few hundred)


def dump_outputs(dirname, arrays, rank, world):
    """--dump-outputs: what the last timed step returned to its caller, as DIR/<name>.npy (float32, as computed).  An array over
    its share of DUMP_BYTES is replaced by a fixed, seeded sample of its rows (axis 0: the utterances of the conv backbones'
    caches; single elements of the flattened array if even one row does not fit) -- <name>_sample.npy, with the sampled row
    numbers in <name>_sample_index.npy (float64).  The share covers the index file and both headers.  With N ranks every rank
    writes its own outputs, suffixed _rank<r>."""
    os.makedirs(dirname, exist_ok=True)
    share = DUMP_BYTES // (world * len(arrays))
    sfx = f"_rank{rank}" if world > 1 else ""
    written = []
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        if a.nbytes + NPY_HEADER_BYTES > share:
            budget = share - 2 * NPY_HEADER_BYTES                 # the sample and its index file
            if a.nbytes // a.shape[0] + 8 > budget:
                a = a.reshape(-1)
            n = budget // (a.nbytes // a.shape[0] + 8)               # each row costs its bytes + one float64 index
            idx = np.sort(np.random.default_rng(0).choice(a.shape[0], size=n, replace=False))
            written.append(os.path.join(dirname, f"{name}_sample_index{sfx}.npy"))
            np.save(written[-1], idx.astype(np.float64))
            a, name = a[idx], name + "_sample"
        written.append(os.path.join(dirname, f"{name}{sfx}.npy"))
        np.save(written[-1], a)
    total = sum(os.path.getsize(f) for f in written)
    assert total <= DUMP_BYTES // world, f"--dump-outputs wrote {total} bytes, over the {DUMP_BYTES // world} of this rank"


def secondary(torch, init_model, pack, synth, dev, name, B, T, steps=30, score_only=False, precision="default"):
    cfg, _, m = build_model(torch, init_model, pack, synth, name, dev, precision)
    x = torch.from_numpy(synth.synth_feats(B, T, cfg["input_dim"], seed=7)).to(dev)
    fn = (lambda: m.posteriors(x)) if score_only else (lambda: m(x))
    ts = time_steps(torch, fn, steps, 5)
    what = "posteriors only (out_cache = NULL)" if score_only else "forward"
    med = float(np.median(ts))
    out = {"workload": f"{name} {what}, {B} x 1-s utterances, T={T}", "value": round(B / med * 1e3, 1),
           "unit": "utts/s", "step_ms": pct(ts), "steps": steps, "precision": precision}
    if name in FLOP_PER_UTT and not score_only:                      # its own roofline (BASELINE config 2 is this model)
        prec = {"default": "f16x3"}.get(precision, precision)
        if prec != "f32" and m.effective_precision() != prec:        # (a mode this shape has no kernel for runs f16x3 / f32)
            prec = m.effective_precision()
            out["precision_effective"] = prec
        roof = mfma_roofline(name, B, med, prec)
        roof["kernel_ms_note"] = "median step of this loop (HIP events per group of launches)"
        attach_profile(roof, name, B, prec)
        out["roofline"] = roof
    return out


def stream_latency(torch, init_model, pack, synth, dev, name, B, chunk=10, n=1000):
    """n consecutive chunks of one set of streams with the carried cache; every chunk between two HIP events."""
    cfg, _, m = build_model(torch, init_model, pack, synth, name, dev)
    x = torch.from_numpy(synth.synth_feats(B, chunk, cfg["input_dim"], seed=3)).to(dev)
    y, c = m(x)
    t_pre = time.perf_counter()                                       # steady clocks first (see --preheat)
    while time.perf_counter() - t_pre < 0.3:
        for _ in range(50):
            y, c = m(x, c)
        torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    t0 = time.perf_counter()
    for a, b in ev:
        a.record()
        y, c = m(x, c)
        b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / n
    ts = [a.elapsed_time(b) * 1e3 / chunk for a, b in ev]            # us per frame, GPU side
    out = {"streams": B, "chunks": n}
    out.update({k: round(v, 3) for k, v in pct(ts).items()})
    out["wall_us_per_frame"] = round(wall * 1e6 / chunk, 3)           # host launch path included
    return out


def cpu_stream_latency(cfg, sd, chunk=10, n=200):
    """The reference's CPU operators on the same 10-frame chunks, B = 1 (200 chunks, median)."""
    import torch
    from oracle import torch_ref
    from wekws_amd.utils import synth
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    x = torch.from_numpy(synth.synth_feats(1, chunk, cfg["input_dim"], seed=3))
    avail = torch.get_num_threads()
    best = None
    for th in (1, 4, 16):
        if th > avail:
            continue
        torch.set_num_threads(th)
        y, c = torch_ref.forward(cfg, tsd, x)
        for _ in range(10):
            y, c = torch_ref.forward(cfg, tsd, x, c)
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            y, c = torch_ref.forward(cfg, tsd, x, c)
            ts.append((time.perf_counter() - t0) * 1e6 / chunk)
        med = float(np.median(ts))
        if best is None or med < best["median"]:
            best = {"median": round(med, 2), "p10": round(float(np.percentile(ts, 10)), 2),
                    "p90": round(float(np.percentile(ts, 90)), 2), "threads": th, "chunks": n}
    torch.set_num_threads(avail)
    return best


def physical_cores():
    """One hardware thread per physical core of the CPUs this process may use (sysfs thread_siblings_list)."""
    allowed = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else list(range(os.cpu_count() or 1))
    seen, firsts = set(), []
    for c in allowed:
        try:
            sib = open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list").read().strip()
        except OSError:
            sib = str(c)
        if sib not in seen:
            seen.add(sib)
            firsts.append(c)
    return firsts


def cpu_worker(model_name, threads, T, budget_s):
    """Worker process of cpu_baseline's pinned rows (bench.py --cpu-worker ...): started with OMP_PROC_BIND=close,
    OMP_PLACES=cores, OMP_NUM_THREADS=threads and its affinity already restricted to `threads` physical cores."""
    import torch
    from oracle import torch_ref
    from wekws_amd import pack
    from wekws_amd.utils import synth
    cfg = dict(synth.MODEL_CONFIGS[model_name])
    tsd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(pack.model_spec(cfg), 1234).items()}
    torch.set_num_threads(threads)
    nb = 128 if threads <= 4 else 1024
    x = torch.from_numpy(synth.synth_feats(nb, T, cfg["input_dim"], seed=0))
    torch_ref.forward(cfg, tsd, x)
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < budget_s:
        torch_ref.forward(cfg, tsd, x)
        n += nb
    print(json.dumps({"threads": threads, "batch": nb, "utts": n, "seconds": round(time.perf_counter() - t0, 2),
                      "torch_threads": torch.get_num_threads()}))


def cpu_pinned_rows(model_name, T, budget_s=3.0):
    """utts/s with ONE OpenMP thread pinned per physical core, for a few core counts (the unpinned "all hardware threads"
    row loses to one thread on a busy 256-thread host: oversubscription and migration, not the reference's best)."""
    cores = physical_cores()
    rows = {}
    for n in sorted({c for c in (4, 16, 64, len(cores)) if 0 < c <= len(cores)}):
        env = dict(os.environ, OMP_NUM_THREADS=str(n), OMP_PROC_BIND="close", OMP_PLACES="cores", MKL_NUM_THREADS=str(n))
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", f"{model_name},{n},{T},{budget_s}"]

        def pin(sel=cores[:n]):
            os.sched_setaffinity(0, sel)
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120, preexec_fn=pin)
            rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            rows[n] = {"threads": n, "batch": rec["batch"], "utts_per_s": round(rec["utts"] / rec["seconds"], 1),
                       "sample_s": rec["seconds"]}
        except Exception as e:                                # (a box that forbids affinity changes: report, do not fail)
            rows[n] = {"threads": n, "error": str(e)[:200]}
    return rows, len(cores)


def cpu_sharded_row(model_name, T, budget_s=4.0, threads=4, max_procs=64):
    """The CPU deployment that corresponds to the GPU ranks: P worker PROCESSES, each with `threads` OpenMP threads pinned to
    its own physical cores, every process running its own share of the utterances (no cross-process traffic, like the
    forward across GPUs).  utts/s = all utterances / the slowest worker's time."""
    cores = physical_cores()
    P = min(max_procs, len(cores) // threads)
    if P < 2:
        return None
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), OMP_PROC_BIND="close", OMP_PLACES="cores", MKL_NUM_THREADS=str(threads))
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", f"{model_name},{threads},{T},{budget_s}"]
    procs = []
    try:
        for i in range(P):
            sel = cores[i * threads:(i + 1) * threads]
            procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True,
                                          preexec_fn=(lambda s=sel: os.sched_setaffinity(0, s))))
        utts, secs = 0, 0.0
        for pr in procs:
            out, _ = pr.communicate(timeout=180)
            rec = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            utts += rec["utts"]
            secs = max(secs, rec["seconds"])
        return {"processes": P, "threads_per_process": threads, "cores": P * threads, "utts_per_s": round(utts / secs, 1),
                "sample_s": round(secs, 2)}
    except Exception as e:                                    # (report, do not fail the bench line)
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
        return {"processes": P, "threads_per_process": threads, "error": str(e)[:200]}


def cpu_baseline(cfg, sd, T, idim, model_name="ds_tcn_h256"):
    """The reference's CPU path on this box's host cores, bounded to ~25 s: oracle/torch_ref.py issues the
    ATen CPU operator sequence of the reference's PyTorch forward (the reference tree does not travel to the GPU box)."""
    import torch
    from oracle import torch_ref
    from wekws_amd.utils import synth
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    avail = torch.get_num_threads()
    ncpu = os.cpu_count() or avail

    def rate(nb, budget_s, cap):
        x = torch.from_numpy(synth.synth_feats(nb, T, idim, seed=0))
        torch_ref.forward(cfg, tsd, x)  # warm-up
        t0, n = time.perf_counter(), 0
        while True:
            torch_ref.forward(cfg, tsd, x)
            n += nb
            el = time.perf_counter() - t0
            if el > budget_s or n >= cap:
                return n, el

    def bsz(threads):                                         # batch per forward: cache-sized for a few threads
        return 128 if threads <= 4 else 1024

    rows = {}
    torch.set_num_threads(avail)                              # all cores torch uses by default, B = 1024 batches
    n, el = rate(1024, 4.0, 10 * 1024)
    rows["all_cores"] = {"threads": int(avail), "batch": 1024, "utts_per_s": round(n / el, 1), "sample_s": round(el, 1)}
    torch.set_num_threads(1)                                  # one core
    n, el = rate(128, 4.0, 1024)
    rows["one_core"] = {"threads": 1, "batch": 128, "utts_per_s": round(n / el, 1), "sample_s": round(el, 1)}
    sweep = {}
    for th in sorted({t for t in (1, 4, 8, 16, 32, 64) if t <= avail}):   # (shared hosts: more threads is often slower)
        torch.set_num_threads(th)
        n, el = rate(bsz(th), 1.5, 4096)
        sweep[th] = round(n / el, 1)
    cores = max(sweep, key=sweep.get) if sweep else avail
    torch.set_num_threads(cores)
    n, el = rate(bsz(cores), 8.0, 64 * 1024)
    torch.set_num_threads(avail)
    pinned, nphys = cpu_pinned_rows(model_name, T)
    rows["pinned_one_thread_per_physical_core"] = pinned
    value, vcores, how = n / el, int(cores), f"{cores} unpinned threads, the best of a sweep {sweep}"
    for k, r in pinned.items():
        if r.get("utts_per_s", 0) > value:
            value, vcores, how = r["utts_per_s"], int(k), (f"{k} threads pinned one per physical core "
                                                           "(OMP_PROC_BIND=close, OMP_PLACES=cores, affinity set)")
    sharded = cpu_sharded_row(model_name, T)
    if sharded:
        rows["process_sharded"] = sharded
        if sharded.get("utts_per_s", 0) > value:
            value, vcores = sharded["utts_per_s"], int(sharded["cores"])
            how = (f"{sharded['processes']} processes x {sharded['threads_per_process']} pinned threads, utterances split over the "
                   "processes as over GPU ranks")
    # spread of the reported row across repeats (11.2 k / 13.4 k / 15.1 k across boxes and sessions)
    reps = [value]
    if sharded and sharded.get("utts_per_s", 0) >= value:
        for _ in range(3):
            r = cpu_sharded_row(model_name, T, budget_s=3.0)
            if r and r.get("utts_per_s"):
                reps.append(r["utts_per_s"])
    spread = {"samples": len(reps), "median": round(float(np.median(reps)), 1), "p10": round(float(np.percentile(reps, 10)), 1),
              "p90": round(float(np.percentile(reps, 90)), 1), "min": round(min(reps), 1), "max": round(max(reps), 1)}
    compact = {"value": round(value, 1), "unit": "utts/s", "cores": vcores, "kind": "port",
               "sample": f"{model_name}, batches of T={T} utterances through oracle/torch_ref.py (the reference's PyTorch CPU operator "
                         f"sequence, fp32), 3-8 s per row, ~25 s in all; best row reported: {how}",
               "host": f"{ncpu} hardware threads / {nphys} physical cores",
               "one_core": rows["one_core"]["utts_per_s"],
               "port_vs_reference": "profiles/r06_cpu_port_vs_reference.json (build box: same outputs, 0.9-1.1x the real KWSModel.forward)"}
    return compact, {"spread": spread, "rows": rows}


def self_launch(args, script=None, need_gpus=True):
    """--gpus N without a launcher: spawn the N ranks ourselves (what the driver's torch.distributed.run line does).
    `script` / `need_gpus`: tests/tools/bench_stub.py drives this launcher with CPU ranks."""
    import torch
    if need_gpus and not getattr(args, "share_gpu", False) and torch.cuda.device_count() < args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus}: only {torch.cuda.device_count()} GPU(s) visible")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(script or __file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--model", default="ds_tcn_h256")
    ap.add_argument("--batch", type=int, default=1024, help="utterances per GPU")
    ap.add_argument("--preheat", type=float, default=0.5,
                    help="seconds of the same forward before the W warm-up steps: an idle MI355X runs its first ~0.25 s "
                         "of work at lower clocks (measured: 0.293 ms per step after 10 steps, 0.244 ms after 1000)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything else: the W + K steps on the idle GPU (value_no_preheat), the step-time "
                         "spread, the CPU baseline, the secondary workloads and streaming latency, with the verbose records "
                         "in the side file (--extras-out); a plain run times the K steps alone")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-worker", default=None, help=argparse.SUPPRESS)   # model,threads,T,seconds: see cpu_pinned_rows
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the secondary workloads (the contract line is the same)")
    ap.add_argument("--extras-out", default=None, help="where the extras go (default gpurun_out/bench_extras.json)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="PLUMBING TEST ONLY (tests/test_hip_bench.py on a 1-GPU box): all ranks use cuda:0 and talk over gloo, so "
                         "that every multi-rank statement of this file runs on a GPU at least once; the line is marked "
                         "`test_mode` and is not a measurement")
    ap.add_argument("--precision", default="default", choices=["default", "f32", "f16x3", "f16"],
                    help="matrix arithmetic of `value` (enum wekws_hip_precision); default = f16x3 with block floating "
                         "point (fp32-level accuracy at any operand scale); the f32 number is always reported beside it")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step computed (posteriors, streaming cache; seeded inputs) to DIR/<name>.npy, "
                         "<= 64 MB in all (a seeded sample of the rows of a larger array): two builds compare output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.cpu_worker:
        name, th, tt, bud = args.cpu_worker.split(",")
        return cpu_worker(name, int(th), int(tt), float(bud))

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))

    import torch
    import torch.distributed as dist
    from wekws_amd import pack, parallel
    from wekws_amd.utils import synth

    rank, world, local = parallel.init_distributed("gloo" if args.share_gpu else None)
    if args.share_gpu:
        local = 0
    if world != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU")
    from wekws_amd.model.kws_model import init_model
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU (the product path has no CPU fallback)")
    if torch.cuda.device_count() <= local or (not args.share_gpu and torch.cuda.device_count() < min(args.gpus, world)):
        raise SystemExit(f"bench.py --gpus {args.gpus}: rank {rank} (LOCAL_RANK {local}) sees {torch.cuda.device_count()} GPU(s); "
                         "one rank per GPU needs at least as many visible devices (check HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    comm_dev = torch.device("cpu") if args.share_gpu else dev     # where the job's few collective payloads live (gloo: host)

    cfg = dict(synth.MODEL_CONFIGS[args.model])
    T, idim, B = 98, cfg["input_dim"], args.batch
    model = init_model(cfg)
    sd = None
    if rank == 0:  # only rank 0 "loads the checkpoint"; the others receive the weights over RCCL
        sd = synth.synth_state_dict(pack.model_spec(cfg), 1234)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(dev).eval().set_precision(args.precision)
    torch.cuda.synchronize()
    t_bc = time.perf_counter()
    parallel.broadcast_weights(model, src=0, device=comm_dev)   # the job's ONE collective (RCCL over xGMI when world > 1)
    torch.cuda.synchronize()
    t_bc = time.perf_counter() - t_bc
    bc_bytes = 4 * sum(int(t.numel()) for t in model.state_dict().values() if t.is_floating_point())
    model.freeze()
    prec = {"default": "f16x3"}.get(args.precision, args.precision)

    x = torch.from_numpy(synth.synth_feats(B, T, idim, seed=100 + rank)).to(dev)
    if args.full:
        # The contract's W + K steps as the idle GPU runs them, BEFORE any preheat (`value_no_preheat`: the literal reading
        # of "W warm-up steps, then K timed steps"; the clocks are still ramping, so it is the lower of the two readings).
        for _ in range(args.warmup):
            y, cache = model(x)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            y, cache = model(x)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        cold = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=comm_dev)
        if world > 1:
            dist.all_reduce(cold, op=dist.ReduceOp.MAX)
        cold_s = float(cold.item())
    # bring the GPU out of its idle power state (clock ramp) with the workload itself; then the contract's W + K steps
    t_pre, n_pre = time.perf_counter(), 0
    while time.perf_counter() - t_pre < args.preheat:
        for _ in range(50):
            y, cache = model(x)
        torch.cuda.synchronize()
        n_pre += 50
    for _ in range(args.warmup):
        y, cache = model(x)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()                                              # HIP events on the launch stream, around the K steps
    for i in range(args.steps):
        y, cache = model(x)
    ev1.record()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    kern_ms = ev0.elapsed_time(ev1) / args.steps              # average launch duration over the timed region
    if args.full:
        # spread of the step time, outside the timed region: >= 50 samples, each GROUP launches between two HIP events
        keep = {}

        def one_step():                   # outputs stay bound across the next call, as `y, cache = model(x)` above and
            keep["o"] = model(x)          # `logits, _ = model(feats)` in score.py:125 do: the caching allocator then
                                          # alternates two 110 MB cache buffers (dropping the result at once recycles ONE
                                          # buffer, whose rewrites hit the memory-side cache: 0.24 instead of 0.28 ms)
        step_ms = time_steps(torch, one_step, max(50, args.steps), 0)
        # the same steps with the result dropped at once (one output buffer recycled by the caching allocator)
        step_ms_single = time_steps(torch, lambda: model(x), max(50, args.steps), 0)
    rank_rates, bc_ms_max = [B * args.steps / elapsed], t_bc * 1e3
    props = torch.cuda.get_device_properties(dev)
    place = {"rank": rank, "local_rank": local, "device": f"cuda:{local}", "name": props.name,
             "cus": int(props.multi_processor_count), "host": socket.gethostname(), "pid": os.getpid()}
    places = [place]
    if world > 1:
        places = [None] * world
        dist.all_gather_object(places, place)
    if world > 1:
        mine = torch.tensor([elapsed, t_bc], dtype=torch.float64, device=comm_dev)
        allr = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        rank_rates = [B * args.steps / float(t[0].item()) for t in allr]
        bc_ms_max = max(float(t[1].item()) for t in allr) * 1e3
        elapsed = max(float(t[0].item()) for t in allr)       # MAX over ranks
    assert torch.isfinite(y).all()
    if args.dump_outputs:                                     # y, cache: still the outputs of the last timed step
        dump_outputs(args.dump_outputs, {"posteriors": y, "cache": cache}, rank, world)

    if rank == 0:
        value = B * world * args.steps / elapsed
        out = {
            "metric": "1-sec utterances/sec (40-d fbank -> DS-TCN posteriors), whole job; per-frame streaming latency in `latency`",
            "value": round(value, 1), "unit": "utts/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,
            "dtype": {"f32": "f32 (exact-f32 MFMA)",
                      "f16": "f32 in/out/accumulate; fp16 operands, one MFMA per product (reduced precision, ~1e-3)"}.get(
                          prec, "f32 in/out/accumulate; products as 3 x fp16 MFMA on block-floating hi/lo-split operands "
                                "(fp32-level accuracy at any operand scale)"),
            "data": "synthetic",
            "config": {"workload": f"{args.model} forward, {B} x 1-s utterances per GPU, T=98 frames x {idim}-d fbank in "
                                   f"HBM -> (B,98,{cfg['output_dim']}) posteriors + the streaming cache",
                       "batch_per_gpu": B, "frames": T, "feat_dim": idim, "precision": prec,
                       "preheat_s": args.preheat, "preheat_steps": n_pre,
                       "parallelism": f"utterance-parallel x{world}"},
        }
        # everything that is not the contract goes to the side file / earlier stdout lines (see emit()); --full only
        extra = {}
        if args.full:
            extra["lib_sha16"] = lib_sha16()
            out["value_no_preheat"] = round(B * world * args.steps / cold_s, 1)
            out["ms_per_step_no_preheat"] = round(cold_s / args.steps * 1e3, 4)
            out["step_ms"] = dict(pct(step_ms), samples=len(step_ms), launches_per_sample=GROUP)
            extra["value_single_output_buffer"] = {
                "value": round(B * world / float(np.median(step_ms_single)) * 1e3, 1), "unit": "utts/s",
                "step_ms": pct(step_ms_single),
                "note": "result dropped at once: ONE 110 MB cache buffer is recycled and its rewrites hit the 256 MB "
                        "memory-side cache; `value` / `step_ms` keep the result bound across the next call (two buffers "
                        "alternate), as score.py:125 does"}
            extra["value_no_preheat_note"] = (f"the same {args.warmup} + {args.steps} steps taken first, on the idle GPU, before "
                                              "the preheat (wall clock, barriers + synchronize on both sides, MAX over ranks)")
        if world > 1:
            out["comm"] = {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                           "collectives_in_timed_region": 0, "broadcast_bytes": bc_bytes,
                           "broadcast_ms_max_over_ranks": round(bc_ms_max, 3),
                           "note": "one broadcast of the weights before the timed region (RCCL over xGMI for backend nccl); "
                                   "the forward itself has no collective"}
            out["per_rank_utts_per_s"] = {"min": round(min(rank_rates), 1), "max": round(max(rank_rates), 1),
                                          "all": [round(r, 1) for r in rank_rates]}
            out["comm"]["ranks"] = [f"r{p['rank']}:{p['device']}@{p['host']}/{p['pid']} {p['cus']}cu" for p in places]
            extra["ranks"] = places
            if args.share_gpu:
                out["test_mode"] = "--share-gpu: all ranks on cuda:0 over gloo (plumbing test, NOT a measurement)"
            else:
                assert len({(p["host"], p["device"]) for p in places}) == world, f"two ranks share a GPU: {places}"
        if args.model in FLOP_PER_UTT:
            roof = mfma_roofline(args.model, B, kern_ms, prec)
            roof["kernel_ms_note"] = "HIP events around the K timed steps / K"
            attach_profile(roof, args.model, B, prec)
            extra["roofline_verbose"] = roof
            out["roofline"] = compact_roofline(roof)
        extras = args.full and world == 1 and args.model == "ds_tcn_h256" and not args.no_extras
        if extras:
            if prec != "f32":        # the same batch at the reference's own arithmetic
                ts = time_steps(torch, lambda m=build_model(torch, init_model, pack, synth, args.model, dev, "f32")[2]: m(x), 30, 5)
                med = float(np.median(ts))
                roof32 = mfma_roofline(args.model, B, med, "f32")
                attach_profile(roof32, args.model, B, "f32")
                extra["f32"] = {"workload": out["config"]["workload"], "precision": "f32", "value": round(B / med * 1e3, 1),
                              "unit": "utts/s", "step_ms": pct(ts), "steps": 30, "roofline": roof32}
            # BASELINE.json configs[1] words the single-GPU case as "MDTC ... batch 1024 x 1 s" while its metric names
            # the DS-TCN: the DS-TCN is `value`; the MDTC 4x4 h64 recipe on the same batch is reported beside it.
            extra["also"] = secondary(torch, init_model, pack, synth, dev, "mdtc_h64", B, T)
            extra["score_only"] = secondary(torch, init_model, pack, synth, dev, "ds_tcn_h256", B, T, score_only=True)
            # BASELINE config 3's model as a batch (the layer wavefront, gru_pipe.hip.h) and the small recipes (hey_snips
            # ds_tcn.yaml, mdtc_small.yaml: the register-resident kernels of round 4), each with its own roofline
            extra["gru"] = secondary(torch, init_model, pack, synth, dev, "gru_2x128", B, T)
            extra["small_recipes"] = {n: secondary(torch, init_model, pack, synth, dev, n, B, T) for n in ("ds_tcn_h64", "mdtc_small")}
            # ---- BASELINE.json configs 4 and 5 as one GPU sees them
            extra["config4_shard"] = {
                "note": "configs[3] shards B = 8192 over 8 GPUs (1024 per GPU = `value` / `also`); these are 8192 utterances in ONE "
                        "launch on one GPU -- eight resident rounds instead of one, the throughput figure of the kernels",
                "ds_tcn_h256": secondary(torch, init_model, pack, synth, dev, "ds_tcn_h256", 8192, T, steps=20),
                "mdtc_h64": secondary(torch, init_model, pack, synth, dev, "mdtc_h64", 8192, T, steps=20),
                "small_recipes": {n: secondary(torch, init_model, pack, synth, dev, n, 8192, T, steps=20) for n in ("ds_tcn_h64", "mdtc_small")}}
            extra["config5"] = {
                "note": "configs[4]: 12-class MDTC h64 + GlobalClassifier, fp16 weights + ONE fp16 MFMA per pointwise product "
                        "(precision 'f16': posterior error ~1e-3, stated in tests/test_hip_parity.py::test_precision_f16_mode), "
                        "roofline against the full 2500 TF; the default precision (f16x3, <= 1e-4) beside it",
                "f16_B1024": secondary(torch, init_model, pack, synth, dev, "mdtc_h64_global12", 1024, T, precision="f16"),
                "f16_B8192": secondary(torch, init_model, pack, synth, dev, "mdtc_h64_global12", 8192, T, steps=20, precision="f16"),
                "default_B1024": secondary(torch, init_model, pack, synth, dev, "mdtc_h64_global12", 1024, T),
                "default_B8192": secondary(torch, init_model, pack, synth, dev, "mdtc_h64_global12", 8192, T, steps=20)}
            # ---- the other half of the metric: per-frame streaming latency, 10-frame chunks, carried cache
            lat = {"unit": "us per frame (10-frame chunks; median / p10 / p90 over 1000 consecutive chunks, HIP events)"}
            for name in ("gru_2x128", "ds_tcn_h256", "mdtc_h64"):
                lat[name] = {f"B{b}": stream_latency(torch, init_model, pack, synth, dev, name, b) for b in (1, 256)}
            extra["latency"] = lat
            # ... and with the Android caller's chunk size (80 frames, runtime/android/app/src/main/cpp/wekws.cc:84-97; the
            # shipped model is the DS-TCN h64 shape): chunks with a carried cache run the register-resident kernels'
            # context variants since round 5
            lat80 = {"unit": "us per frame (80-frame chunks with the carried cache; median / p10 / p90 over 300 consecutive chunks)"}
            for name in ("ds_tcn_h64", "ds_tcn_h256", "mdtc_h64"):
                lat80[name] = {f"B{b}": stream_latency(torch, init_model, pack, synth, dev, name, b, chunk=80, n=300) for b in (1, 256)}
            extra["latency_chunk80"] = lat80
            # ---- HBM-bound kernels
            other = []
            Bs = 4096
            cfgs, _, ms = build_model(torch, init_model, pack, synth, "ds_tcn_h256", dev)
            xs = torch.from_numpy(synth.synth_feats(Bs, 10, 40, seed=3)).to(dev)
            _, cs = ms(xs)
            state = {"c": cs}

            def step_stream():
                _, state["c"] = ms(xs, state["c"])
            ts = time_steps(torch, step_stream, 50, 10)
            by = Bs * (2 * CACHE_BYTES_PER_UTT + 10 * 40 * 4 + 10 * 2 * 4)
            med = float(np.median(ts))
            other.append({"kernel": "ds256_stream_kernel", "workload": f"{Bs} DS-TCN h256 streams x one 10-frame chunk (cache in + out)",
                          "bound": "hbm", "algorithmic_bytes_per_launch": by, "achieved": round(by / (med * 1e-3) / 1e9, 1),
                          "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(by / (med * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                          "step_ms": pct(ts), "stream_chunks_per_s": round(Bs / med * 1e3, 1)})
            from wekws_amd.frontend import Fbank
            fb = Fbank(num_bins=40, device=dev)
            pcm = torch.from_numpy(synth.synth_pcm(1024, 16000, seed=0, kind="noise")).to(dev)
            ts = time_steps(torch, lambda: fb(pcm), 50, 10)
            by = 1024 * (16000 * 4 + 98 * 40 * 4)
            med = float(np.median(ts))
            other.append({"kernel": "fbank_kernel", "workload": "1024 x 1 s of 16 kHz PCM (f32) -> (1024, 98, 40) log-mel",
                          "bound": "hbm", "algorithmic_bytes_per_launch": by, "achieved": round(by / (med * 1e-3) / 1e9, 1),
                          "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(by / (med * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                          "step_ms": pct(ts), "utts_per_s": round(1024 / med * 1e3, 1),
                          "note": "instruction-bound radix-4 FFT + mel slots (~2.6 MFLOP per utterance), not HBM-bound"})
            extra["rooflines_other"] = other
            # ---- the whole device-side pipeline: PCM in HBM -> log-mel -> posteriors + cache (two launches per step)
            ts = time_steps(torch, lambda: model(fb(pcm)), 50, 10)
            med = float(np.median(ts))
            extra["audio_to_posteriors"] = {"workload": "1024 x 1 s of 16 kHz PCM (f32, in HBM) -> fbank_kernel -> ds_tcn_h256 forward",
                                          "value": round(1024 / med * 1e3, 1), "unit": "utts/s", "step_ms": pct(ts), "steps": 50,
                                          "pcie_note": "with the PCM coming over PCIe Gen5 x16 (~63 GB/s, 64 KB per utterance) the "
                                                       "host link caps the pipeline at ~0.98 M utt/s (f32 PCM; int16: ~1.97 M)"}
        if extras:                            # a few numbers of the extras in the contract line (the rest: extras_file)
            lat, l80 = extra["latency"], extra["latency_chunk80"]
            out["summary"] = {
                "unit": "utts/s at B=1024 unless said; latency = us per frame, median, streaming with the carried cache",
                "f32": {"value": extra["f32"]["value"], "frac_of_157.3TF": extra["f32"]["roofline"]["frac"]},
                "mdtc_h64": {"value": extra["also"]["value"], "frac": extra["also"]["roofline"]["frac"]},
                "gru_2x128": {"value": extra["gru"]["value"], "frac": extra["gru"]["roofline"]["frac"]},
                "B8192": {n: extra["config4_shard"][n]["value"] for n in ("ds_tcn_h256", "mdtc_h64")},
                "config5_f16_B8192": {"value": extra["config5"]["f16_B8192"]["value"],
                                      "frac_of_2500TF": extra["config5"]["f16_B8192"]["roofline"]["frac"]},
                "latency_chunk10": {n: {b: lat[n][b]["median"] for b in ("B1", "B256")} for n in ("gru_2x128", "ds_tcn_h256", "mdtc_h64")},
                "latency_chunk80": {n: {b: l80[n][b]["median"] for b in ("B1", "B256")} for n in ("ds_tcn_h64", "ds_tcn_h256", "mdtc_h64")},
                "hbm_bound": {o["kernel"]: {"ms": o["step_ms"]["median"], "frac": o["frac"]} for o in extra["rooflines_other"]},
                "audio_to_posteriors": extra["audio_to_posteriors"]["value"]}
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"], extra["cpu_baseline_detail"] = cpu_baseline(cfg, sd, T, idim, args.model)
            if extras:
                for name in ("gru_2x128", "ds_tcn_h256", "mdtc_h64"):
                    c2 = dict(synth.MODEL_CONFIGS[name])
                    extra["latency"][name]["cpu"] = cpu_stream_latency(c2, synth.synth_state_dict(pack.model_spec(c2), 1234))
        if args.full:
            emit(out, extra, args.extras_out)
        else:
            print_line(out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
