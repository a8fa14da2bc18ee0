"""Runs the GPU cases of KWSModel.forward_streams / wekws_hip_forward_streams with the TEST build of the library
(libwekws_hip_hooks.so, for wekws_hip_debug_route_trace), for tests/test_hip_forward_streams.py.  Run as a subprocess with
WEKWS_HIP_LIB pointing at it:

    python tests/tools/forward_streams_cases.py [section ...]      (schedule, packed, nonfinite, refusals, pipeline; default all)

One JSON record per line on stdout -- every figure a test asserts on, measured here and judged there --, then OK: exit code 0
when every case was MADE.

The schedule: a pool of 7 streams, three consecutive calls of 5 rows, ids permuted between calls.  It holds T = 1, T = 16 (the whole
tile of ds256_stream), a skipped row (0 and -1 frames), a stream left out of the middle call (5), streams present in all three
(6 and 3: their parity flips twice), a stream that enters late (4) and a stream reset between the second and the third call (0)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import kws_oracle  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import route_matrix as rm  # noqa: E402
from wekws_amd import _capi, pack  # noqa: E402
from wekws_amd.ctc import StreamingKeywordSpotter  # noqa: E402
from wekws_amd.frontend import StreamingFrontEnd  # noqa: E402
from wekws_amd.model.kws_model import StreamCachePool, init_model  # noqa: E402
from wekws_amd.stream import BatchedKeyWordSpotter  # noqa: E402
from wekws_amd.utils import synth  # noqa: E402

STREAMS, TCAP, SENTINEL = 7, 16, 777.0
SCHEDULE = [  # (ids, frames, streams reset BEFORE the call)
    ([6, 2, 0, 5, 3], [10, 0, 3, 16, 1], []),
    ([3, 0, 6, 2, 4], [1, 16, 7, -1, 5], []),
    ([5, 6, 3, 0, 2], [4, 16, 9, 2, 1], [0]),
]
MODELS = {  # name -> (config name, softmax, expected plan kind, the trace's path)
    "ds_tcn_h256": ("ds_tcn_h256", False, "ds256_stream", 1),
    "fsmn_ctc300": ("fsmn_ctc300", True, "fsmn_f16", 4),
    "mdtc_h64": ("mdtc_h64", False, "grouped", 1),
    "gru_2x128": ("gru_2x128", False, "grouped", 3),
}


def emit(**rec):
    print(json.dumps(rec), flush=True)


def trace(lib, n=8):
    out = (ctypes.c_int * (2 + 9 * n))()
    k = lib.wekws_hip_debug_route_trace(out, n)
    return out[0], out[1], [list(out[2 + 9 * i:11 + 9 * i]) for i in range(k)]


def build(name, seed=1234):
    cfg = dict(synth.MODEL_CONFIGS[name])
    sd = synth.synth_state_dict(pack.model_spec(cfg), seed)
    m = init_model(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return cfg, sd, m.cuda().eval().freeze()


def bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def cache_axis(cfg):
    return 1 if cfg["backbone"]["type"] == "gru" else 0


def bucketed_step(model, cache, axis, x, ids, frames, softmax):
    """The model step as BatchedKeyWordSpotter.forward made it before forward_streams: rows bucketed by frame count, per bucket
    index_select out of a dense cache tensor, the uniform forward, index_copy_ back.  Returns {row: y}."""
    fwd = model.forward_softmax if softmax else model.forward
    groups, ys = {}, {}
    for b, n in enumerate(frames):
        if n > 0:
            groups.setdefault(n, []).append(b)
    for n, rows in sorted(groups.items()):
        ridx = torch.tensor(rows, dtype=torch.long, device=x.device)
        sidx = torch.tensor([ids[b] for b in rows], dtype=torch.long, device=x.device)
        y, c = fwd(x.index_select(0, ridx)[:, :n].contiguous(), cache.index_select(axis, sidx).contiguous())
        cache.index_copy_(axis, sidx, c)
        for j, b in enumerate(rows):
            ys[b] = y[j]
    return ys


def schedule(lib, name):
    """The three calls: per live row its y and its stream's cache after the call against (a) the float64 oracle carried per stream,
    (b) KWSModel.forward on that row alone with the cache the pool held, bit for bit, (c) the bucketed step; the sentinel in every
    byte of y the call must not write; the caches of streams a call skips or leaves out."""
    cname, softmax, _, _ = MODELS[name]
    cfg, sd, model = build(cname)
    axis, yax, cax = cache_axis(cfg), H.y_axis(cfg, softmax), H.cache_axis(cfg)
    per_frame = model._d["head"] in (pack.HEAD["linear"], pack.HEAD["identity"])
    pool = StreamCachePool(model, STREAMS)
    dense = torch.zeros(pack.cache_shape(model._d, STREAMS), dtype=torch.float32, device="cuda")
    ocache = [None] * STREAMS
    fwd = model.forward_softmax if softmax else model.forward
    run = model.forward_softmax_streams if softmax else model.forward_streams
    for ci, (ids, frames, resets) in enumerate(SCHEDULE):
        if resets:
            pool.reset(resets)
            dense.index_fill_(axis, torch.tensor(resets, device="cuda"), 0.0)
            for s in resets:
                ocache[s] = None
        x = torch.from_numpy(synth.synth_feats(len(ids), TCAP, cfg["input_dim"], seed=40 + ci)).cuda()
        before = [pool.read(s) for s in range(STREAMS)]
        y = torch.full((len(ids), TCAP, model.odim) if per_frame else (len(ids), model.odim), SENTINEL, device="cuda")
        run(x, frames, ids, pool, out=y)
        torch.cuda.synchronize()
        path, ntiles, recs = trace(lib)
        after = [pool.read(s) for s in range(STREAMS)]
        yb = bucketed_step(model, dense, axis, x, ids, frames, softmax)
        rec = dict(kind="schedule", model=name, call=ci, path=path, ntiles=ntiles, records=recs, rows=[])
        for b, (s, n) in enumerate(zip(ids, frames)):
            if n <= 0:
                rec["rows"].append(dict(row=b, stream=s, frames=n, y_untouched=bool((y[b] == SENTINEL).all()),
                                        cache_kept=bits_equal(after[s], before[s])))
                continue
            got = y[b, :n] if per_frame else y[b]
            ya, ca = fwd(x[b:b + 1, :n].contiguous(), before[s])
            ry, ocache[s] = kws_oracle.forward(cfg, sd, x[b:b + 1, :n].cpu().numpy(), ocache[s], softmax=softmax, dtype=np.float64)
            ey, ec = (H.tight_error(got.cpu().numpy()[None], ry, yax), H.tight_error(after[s].cpu().numpy(), ocache[s], cax))
            rec["rows"].append(dict(
                row=b, stream=s, frames=n, y_err=ey, cache_err=ec, y_alone=bits_equal(got, ya[0]), cache_alone=bits_equal(after[s], ca),
                y_bucketed=bits_equal(got, yb[b]), cache_bucketed=bits_equal(after[s], dense.select(axis, s).unsqueeze(axis)),
                tail_untouched=bool((y[b, n:] == SENTINEL).all()) if per_frame else True))
        rec["left_out_kept"] = all(bits_equal(after[s], before[s]) for s in range(STREAMS) if s not in ids)
        emit(**rec)


def packed(lib):
    """FSMN, one call of 2 x CUs + 3 rows with frames from {1, 7, 16} in a fixed permutation: two rows per workgroup, partial groups."""
    cfg, sd, model = build("fsmn_ctc300")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * cus + 3
    rng = np.random.default_rng(11)
    frames = [int(v) for v in rng.permutation(np.resize([1, 7, 16], B))]
    ids = [int(v) for v in rng.permutation(B)]
    pool = StreamCachePool(model, B)
    # a carried cache for every stream: one uniform call of 3 frames first
    x0 = torch.from_numpy(synth.synth_feats(B, 3, cfg["input_dim"], seed=7)).cuda()
    model.forward_softmax_streams(x0, [3] * B, list(range(B)), pool)
    c0 = torch.cat([pool.read(s) for s in range(B)], 0)
    x = torch.from_numpy(synth.synth_feats(B, TCAP, cfg["input_dim"], seed=8)).cuda()
    y = torch.full((B, TCAP, model.odim), SENTINEL, device="cuda")
    model.forward_softmax_streams(x, frames, ids, pool, out=y)
    torch.cuda.synchronize()
    path, ntiles, recs = trace(lib)
    c1 = torch.cat([pool.read(s) for s in range(B)], 0)
    cin = c0.index_select(0, torch.tensor(ids, device="cuda"))
    rec = dict(kind="packed", B=B, cus=cus, path=path, ntiles=ntiles, records=recs, uniform={}, tails=True)
    xn, cn = x.cpu().numpy(), cin.cpu().numpy()
    ey = ec = 0.0
    for T in (1, 7, 16):
        rows = [b for b in range(B) if frames[b] == T]
        # the uniform call over ALL rows at T frames: the same kernel instance; the rows of this frame count are compared
        yu, cu = model.forward_softmax(x[:, :T].contiguous(), cin)
        torch.cuda.synchronize()
        _, _, urecs = trace(lib)
        same = all(bits_equal(y[b, :T], yu[b]) and bits_equal(c1[ids[b]], cu[b]) for b in rows)
        rec["uniform"][str(T)] = dict(records=urecs, rows=len(rows), identical=bool(same))
        ry, rc = kws_oracle.forward(cfg, sd, xn[rows, :T], cn[rows], softmax=True, dtype=np.float64)
        sel = torch.tensor(rows, device="cuda")
        ey = max(ey, H.tight_error(y.index_select(0, sel)[:, :T].cpu().numpy(), ry, None))
        ec = max(ec, H.tight_error(c1.index_select(0, torch.tensor([ids[b] for b in rows], device="cuda")).cpu().numpy(), rc, 1))
        rec["tails"] = rec["tails"] and bool((y.index_select(0, sel)[:, T:] == SENTINEL).all())
    rec.update(y_err=ey, cache_err=ec)
    emit(**rec)


def nonfinite(lib, name):
    """One warm call, then one call of 5 rows twice on twin pools: clean, and with a NaN feature in row 1 and a +Inf written into the
    carried cache of row 3's stream.  The poisoned rows against the float64 oracle's classes and values, the others bit for bit."""
    cname, softmax, _, _ = MODELS[name]
    cfg, sd, model = build(cname)
    yax, cax = H.y_axis(cfg, softmax), H.cache_axis(cfg)
    run = model.forward_softmax_streams if softmax else model.forward_streams
    ids, frames = [4, 1, 6, 0, 2], [9, 12, 1, 16, 5]
    xw = torch.from_numpy(synth.synth_feats(5, TCAP, cfg["input_dim"], seed=21)).cuda()
    x = torch.from_numpy(synth.synth_feats(5, TCAP, cfg["input_dim"], seed=22)).cuda()
    xp = x.clone()
    xp[1, 2, 5] = float("nan")
    out = {}
    for tag, xin in (("clean", x), ("poison", xp)):
        pool = StreamCachePool(model, STREAMS)
        run(xw, [10] * 5, ids, pool)
        if tag == "poison":
            c = pool.read(ids[3])
            c.view(-1)[c.numel() // 3] = float("inf")
            pool.write(ids[3], c)
        cin = [pool.read(s) for s in ids]
        y = torch.full((5, TCAP, model.odim), SENTINEL, device="cuda")
        run(xin, frames, ids, pool, out=y)
        torch.cuda.synchronize()
        out[tag] = (y, [pool.read(s) for s in ids], cin)
    (yc, cc, _), (yp, cp, cin) = out["clean"], out["poison"]
    rec = dict(kind="nonfinite", model=name, rows=[])
    for b in range(5):
        n = frames[b]
        if b in (1, 3):
            with np.errstate(all="ignore"):
                ry, rc = kws_oracle.forward(cfg, sd, xp[b:b + 1, :n].cpu().numpy(), cin[b].cpu().numpy(), softmax=softmax, dtype=np.float64)
            rec["rows"].append(dict(row=b, poisoned=True, y_err=H.masked_tight_error(yp[b:b + 1, :n].cpu().numpy(), ry, yax),
                                    cache_err=H.masked_tight_error(cp[b].cpu().numpy(), rc, cax),
                                    nonfinite=int((~np.isfinite(ry)).sum() + (~np.isfinite(rc)).sum())))
        else:
            rec["rows"].append(dict(row=b, poisoned=False, identical=bits_equal(yp[b], yc[b]) and bits_equal(cp[b], cc[b])))
    emit(**rec)


def refusals(lib):
    """Every bad call returns WEKWS_HIP_EINVAL with the row named, launches nothing and changes no stream: a good call behind them
    equals the same call on a twin pool that never saw them."""
    cfg, sd, model = build("ds_tcn_h256")
    _, _, other = build("ds_tcn_h256", seed=99)
    pool, twin, foreign = StreamCachePool(model, STREAMS), StreamCachePool(model, STREAMS), StreamCachePool(other, STREAMS)
    x = torch.from_numpy(synth.synth_feats(5, TCAP, cfg["input_dim"], seed=31)).cuda()
    ids, frames = [6, 2, 0, 5, 3], [10, 4, 3, 16, 1]
    model.forward_streams(x, frames, ids, pool)
    model.forward_streams(x, frames, ids, twin)
    bad = {"repeated id": ([6, 2, 0, 2, 3], frames, 3), "id = max_streams": ([6, 2, STREAMS, 5, 3], frames, 2),
           "frames = Tcap + 1": (ids, [10, 4, 3, 16, TCAP + 1], 4)}
    rec = dict(kind="refusals", calls={})
    y = torch.full((5, TCAP, model.odim), SENTINEL, device="cuda")
    L = _capi.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(m, p, i, f):
        i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)     # noqa: E731
        a, b = i32(i), i32(f)
        rc = L.wekws_hip_forward_streams(m._get_handle(x.device).ptr, p._ptr, x.data_ptr(), 5, TCAP, a.ctypes.data, b.ctypes.data,
                                         y.data_ptr(), 0, stream)
        return rc, _capi.last_error()

    for what, (i, f, row) in bad.items():
        rc, msg = call(model, pool, i, f)
        rec["calls"][what] = dict(rc=rc, message=msg, names_row=f"row {row}" in msg)
    rc, msg = call(model, foreign, ids, frames)
    rec["calls"]["pool of another model"] = dict(rc=rc, message=msg, names_row=True)
    torch.cuda.synchronize()
    rec["y_untouched"] = bool((y == SENTINEL).all())
    ya, yb = model.forward_streams(x, frames, ids, pool, out=y), model.forward_streams(x, frames, ids, twin)
    torch.cuda.synchronize()
    rec["good_call_same"] = all(bits_equal(ya[b, :n], yb[b, :n]) for b, n in enumerate(frames)) and \
        all(bits_equal(pool.read(s), twin.read(s)) for s in range(STREAMS))
    emit(**rec)


def pipeline(lib):
    """BatchedKeyWordSpotter over an FSMN with uneven chunks against the bucketed step written out here, from a twin front end and
    a twin decoder: detections and posteriors, bit for bit."""
    fe = dict(num_bins=40, window="hamming", left=1, right=1, skip=2)
    kws = {"k0": (1, 2), "k1": (7,)}
    spot = dict(min_frames=0, max_frames=40)
    cfg, sd, model = build("fsmn_small", seed=5)
    n_streams = 6
    kw = BatchedKeyWordSpotter(model, kws, 0.0, n_streams, max_chunk=4000, **fe, **spot)
    front = StreamingFrontEnd(n_streams, max_chunk=4000, **fe)
    shift_ms = 1000.0 * front.cfg.fbank.frame_shift / front.cfg.fbank.sample_rate
    dec = StreamingKeywordSpotter(n_streams, kws, 0.0, downsampling=front.skip, frame_shift_ms=shift_ms, **spot)
    dense = torch.zeros(pack.cache_shape(model._d, n_streams), dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(3)
    pcm = rng.integers(-12000, 12000, size=(n_streams, 40000), dtype=np.int16)
    pos = [0] * n_streams
    rec = dict(kind="pipeline", calls=0, rows=0, same_results=True, same_probs=True, frame_counts=[], paths=[], fired=0)
    for c in range(7):
        live = [s for s in range(n_streams) if s // 2 <= c]
        pick = [s for s in live if rng.random() < 0.8] or live[:1]
        ids = [pick[i] for i in rng.permutation(len(pick))]
        chunks = []
        for s in ids:
            n = int(rng.choice([800, 801, 1600, 2399, 3200, 4000]))
            chunks.append(pcm[s, pos[s]:pos[s] + n].copy())
            pos[s] += n
        out, probs, _ = kw.forward(chunks, streams=ids, return_probs=True)
        rec["paths"].append(trace(lib)[0])
        feats, frames = front.push(chunks, streams=ids)
        want = [{} for _ in ids]
        groups = {}
        for b, n in enumerate(frames):
            if n > 0:
                groups.setdefault(n, []).append(b)
        for n, rows in sorted(groups.items()):
            ridx = torch.tensor(rows, dtype=torch.long, device="cuda")
            sidx = torch.tensor([ids[b] for b in rows], dtype=torch.long, device="cuda")
            p, cc = model.forward_softmax(feats.index_select(0, ridx)[:, :n].contiguous(), dense.index_select(0, sidx).contiguous())
            dense.index_copy_(0, sidx, cc)
            res = dec.step(p, streams=[ids[b] for b in rows])
            for j, b in enumerate(rows):
                want[b] = res[j]
                rec["same_probs"] = rec["same_probs"] and bits_equal(probs[b], p[j])
                rec["rows"] += 1
        rec["same_results"] = rec["same_results"] and out == want
        rec["fired"] += sum(int(r.get("state", 0) == 1) for r in out)
        rec["frame_counts"].append(sorted({n for n in frames if n > 0}))
        rec["calls"] += 1
    emit(**rec)


def main():
    lib = rm.type_hooks(_capi.load())
    assert _capi.lib_path().endswith("libwekws_hip_hooks.so"), _capi.lib_path()
    todo = sys.argv[1:] or ["schedule", "packed", "nonfinite", "refusals", "pipeline"]
    if "schedule" in todo:
        for name in MODELS:
            schedule(lib, name)
    if "packed" in todo:
        packed(lib)
    if "nonfinite" in todo:
        for name in ("ds_tcn_h256", "fsmn_ctc300"):
            nonfinite(lib, name)
    if "refusals" in todo:
        refusals(lib)
    if "pipeline" in todo:
        pipeline(lib)
    print("OK")


if __name__ == "__main__":
    main()
