"""Runs the case table of tests/forward_streams_matrix.py on the device with the TEST build of the library
(libwekws_hip_hooks.so), for tests/test_hip_forward_streams_matrix.py.  Run as a subprocess with WEKWS_HIP_LIB pointing at it:

    python tests/tools/forward_streams_matrix_cases.py [section ...]      (fsmn, ds256, grouped, pool, nonfinite; default all)

One JSON record per line on stdout -- every figure a test asserts on, measured here and judged there --, then OK.  The helpers
(build, bucketed_step, bits_equal, trace) are those of tests/tools/forward_streams_cases.py.

Every case starts with one warm call, so that every stream carries a nonzero cache; y is pre-filled with the sentinel; B follows
the device's CU count; EVERY live row goes to the float64 oracle, fed the cache its stream carried."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forward_streams_cases as fc  # noqa: E402  (puts the repository root on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import folded_oracle, kws_oracle  # noqa: E402
from tests import forward_streams_matrix as fm  # noqa: E402
from tests import helpers as H  # noqa: E402
from wekws_amd import _capi, pack  # noqa: E402
from wekws_amd.model.kws_model import StreamCachePool, init_model  # noqa: E402
from wekws_amd.utils import synth  # noqa: E402

SENTINEL = fm.SENTINEL
bits_equal, trace, emit = fc.bits_equal, fc.trace, fc.emit


def build_case(case, seed=1234):
    cfg = fm.case_config(case)
    sd = synth.synth_state_dict(pack.model_spec(cfg), seed)
    m = init_model(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return cfg, sd, m.cuda().eval().freeze()


def feats(B, T, idim, seed):
    return torch.from_numpy(synth.synth_feats(B, T, idim, seed=seed)).cuda()


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def warm(run, pool, n, idim, seed=7):
    """3 frames for every stream of the pool in one call of max_streams rows"""
    run(feats(n, 3, idim, seed), [3] * n, list(range(n)), pool)


def row_errors(got, ref, axis):
    """The tight error of every row on its own (its own channel scales): the worst, and its row"""
    errs = [H.tight_error(got[j:j + 1], ref[j:j + 1], axis) for j in range(got.shape[0])]
    j = int(np.argmax(errs))
    return float(errs[j]), j


# ---------------------------------------------------------------------------------------------------------------------------------
def fsmn_case(lib, case):
    """a. One call on one FSMN instance.  Per frame count: the rows against the float64 oracle, their tails, and bit-identity to
    the uniform call over ALL rows at that count (asserted where its trace shows the same instance).

    The channel scales S_c of the tight bar are taken over the rows of one frame count, as tests/tools/forward_streams_cases.py::packed
    takes them -- not over each row alone: a ONE-frame row on its own scales holds every logit to its own magnitude, and there the
    float32 ORACLE itself misses the bar against the float64 one (4.4e-5 at 2 of 1029 one-frame rows of fsmn_small on the CPU,
    inputs and carried caches of this case; 5.4e-7 with the scales over the rows; 1.3e-6 per row at 15 and 16 frames).  TIGHT_K
    was calibrated on tensors of several frames (tests/helpers.py).  Where a count has one row the two are the same thing."""
    cfg, sd, model = build_case(case)
    ids, frames = fm.frames_of(case, cus())
    B, Tcap, softmax, S = len(ids), case["Tcap"], case["softmax"], len(ids) + 2
    run = model.forward_softmax_streams if softmax else model.forward_streams
    fwd = model.forward_softmax if softmax else model.forward
    yax = H.y_axis(cfg, softmax)
    pool = StreamCachePool(model, S)
    warm(run, pool, S, cfg["input_dim"])
    c0 = torch.cat([pool.read(s) for s in range(S)], 0)
    x = feats(B, Tcap, cfg["input_dim"], 8)
    y = torch.full((B, Tcap, model.odim), SENTINEL, device="cuda")
    run(x, frames, ids, pool, out=y)
    torch.cuda.synchronize()
    path, ntiles, recs = trace(lib)
    c1 = torch.cat([pool.read(s) for s in range(S)], 0)
    idt = torch.tensor(ids, device="cuda")
    cin = c0.index_select(0, idt)
    cout = c1.index_select(0, idt)
    xn, cn, yn, con = x.cpu().numpy(), cin.cpu().numpy(), y.cpu().numpy(), cout.cpu().numpy()
    rec = dict(kind="fsmn", id=case["id"], B=B, cus=cus(), path=path, ntiles=ntiles, records=recs, counts={}, y_err=0.0, cache_err=0.0,
               tails=True, c0_nonzero=bool((c0.abs().amax(dim=(1, 2, 3)) > 0).all()))
    for T in sorted({n for n in frames if n > 0}):
        rows = [b for b in range(B) if frames[b] == T]
        sel = torch.tensor(rows, device="cuda")
        yu, cu = fwd(x[:, :T].contiguous(), cin)
        torch.cuda.synchronize()
        _, _, urecs = trace(lib)
        same = bits_equal(y.index_select(0, sel)[:, :T], yu.index_select(0, sel)) and bits_equal(cout.index_select(0, sel), cu.index_select(0, sel))
        ry, rc = kws_oracle.forward(cfg, sd, xn[rows, :T], cn[rows], softmax=softmax, dtype=np.float64)
        # every row of the count is compared, the channel scales taken over those rows (see the docstring); the worst row on
        # its OWN scales goes into the record for information
        ey, ec = H.tight_error(yn[rows, :T], ry, yax), H.tight_error(con[rows], rc, 1)
        (oy, jy), (oc, jc) = row_errors(yn[rows, :T], ry, yax), row_errors(con[rows], rc, 1)
        rec["counts"][str(T)] = dict(rows=len(rows), uniform=urecs[0][:7], identical=bool(same), y_err=ey, cache_err=ec,
                                     y_own_scale=oy, y_row=rows[jy], cache_own_scale=oc, cache_row=rows[jc])
        rec["y_err"], rec["cache_err"] = max(rec["y_err"], ey), max(rec["cache_err"], ec)
        rec["tails"] = rec["tails"] and bool((y.index_select(0, sel)[:, T:] == SENTINEL).all())
    skipped = [b for b in range(B) if frames[b] <= 0]
    rec["skipped"] = len(skipped)
    rec["skipped_untouched"] = all(bool((y[b] == SENTINEL).all()) and bits_equal(cout[b], cin[b]) for b in skipped)
    rec["left_out_kept"] = all(bits_equal(c1[s], c0[s]) for s in range(S) if s not in ids)
    emit(**rec)


# ---------------------------------------------------------------------------------------------------------------------------------
def ds256_case(lib, case):
    """b. ds256_stream's table-driven variants at precision f16 (one fp16 product: split 0) and with the softmax behind it."""
    cfg, sd, model = build_case(case)
    _, frames = fm.frames_of(case, cus())
    ids, S, Tcap, softmax = [4, 1, 6, 0, 2], fm.STREAMS, case["Tcap"], case["softmax"]
    run = model.forward_softmax_streams if softmax else model.forward_streams
    fwd = model.forward_softmax if softmax else model.forward
    f16 = case["precision"] == "f16"
    desc, blob = pack.pack(cfg, sd)
    pool = StreamCachePool(model, S)
    warm(run, pool, S, cfg["input_dim"])
    before = [pool.read(s) for s in range(S)]
    x = feats(len(ids), Tcap, cfg["input_dim"], 9)
    y = torch.full((len(ids), Tcap, model.odim), SENTINEL, device="cuda")
    run(x, frames, ids, pool, out=y)
    torch.cuda.synchronize()
    path, ntiles, recs = trace(lib)
    after = [pool.read(s) for s in range(S)]
    rec = dict(kind="ds256", id=case["id"], path=path, ntiles=ntiles, records=recs, effective=model.effective_precision(), rows=[])
    for b, (s, n) in enumerate(zip(ids, frames)):
        if n <= 0:
            rec["rows"].append(dict(row=b, frames=n, y_untouched=bool((y[b] == SENTINEL).all()), cache_kept=bits_equal(after[s], before[s])))
            continue
        xa = x[b:b + 1, :n].contiguous()
        ya, ca = fwd(xa, before[s])
        ry, rc = kws_oracle.forward(cfg, sd, xa.cpu().numpy(), before[s].cpu().numpy(), softmax=softmax, dtype=np.float64)
        got, gc = y[b:b + 1, :n].cpu().numpy(), after[s].cpu().numpy()
        row = dict(row=b, frames=n, y_alone=bits_equal(y[b, :n], ya[0]), cache_alone=bits_equal(after[s], ca),
                   tail_untouched=bool((y[b, n:] == SENTINEL).all()))
        if f16:         # the bar of that precision: absolute, in units of max(1, max |ref|)
            ey, ec = folded_oracle.forward(desc, blob, xa.cpu().numpy(), mm_dtype=np.float16, in_cache=before[s].cpu().numpy(), with_cache=True)
            row.update(y_err=H.max_abs(got, ry) / max(1.0, float(np.abs(ry).max())), cache_err=H.max_abs(gc, rc) / max(1.0, float(np.abs(rc).max())),
                       y_emu=H.max_abs(got, ey) / max(1.0, float(np.abs(ey).max())), cache_emu=H.max_abs(gc, ec) / max(1.0, float(np.abs(ec).max())))
        else:
            row.update(y_err=H.tight_error(got, ry, H.y_axis(cfg, softmax)), cache_err=H.tight_error(gc, rc, H.cache_axis(cfg)))
        rec["rows"].append(row)
    rec["left_out_kept"] = all(bits_equal(after[s], before[s]) for s in range(S) if s not in ids)
    emit(**rec)


# ---------------------------------------------------------------------------------------------------------------------------------
def grouped_case(lib, case):
    """c. The three-call schedule of tests/tools/forward_streams_cases.py over any Tcap, frames and config: per live row y and its
    stream's cache against the float64 oracle carried per stream and against the bucketed step, bit for bit."""
    cfg, sd, model = build_case(case)
    S, Tcap, softmax = fm.STREAMS, case["Tcap"], case["softmax"]
    axis, yax, cax = fc.cache_axis(cfg), H.y_axis(cfg, softmax), H.cache_axis(cfg)
    per_frame = model._d["head"] in (pack.HEAD["linear"], pack.HEAD["identity"])
    pool = StreamCachePool(model, S)
    dense = torch.zeros(pack.cache_shape(model._d, S), dtype=torch.float32, device="cuda")
    ocache = [None] * S
    run = model.forward_softmax_streams if softmax else model.forward_streams
    if not per_frame:
        try:
            model.forward_softmax_streams(feats(1, 4, cfg["input_dim"], 1), [4], [0], pool)
            refused = "no error"
        except IndexError as e:
            refused = "IndexError: " + str(e)
        emit(kind="pooled_softmax", id=case["id"], refused=refused, untouched=bool((pool.read(0) == 0).all()))
    calls = [(-1, list(range(S)), [3] * S, [], 3)] + [(ci, ids, case["frames"][ci], resets, Tcap)
                                                         for ci, (ids, resets) in enumerate(fm.SCHEDULE_IDS)]
    for ci, ids, frames, resets, tcap in calls:
        if resets:
            pool.reset(resets)
            dense.index_fill_(axis, torch.tensor(resets, device="cuda"), 0.0)
            for s in resets:
                ocache[s] = None
        x = feats(len(ids), tcap, cfg["input_dim"], 40 + ci)
        before = [pool.read(s) for s in range(S)]
        y = torch.full((len(ids), tcap, model.odim) if per_frame else (len(ids), model.odim), SENTINEL, device="cuda")
        run(x, frames, ids, pool, out=y)
        torch.cuda.synchronize()
        path, ntiles, recs = trace(lib)
        after = [pool.read(s) for s in range(S)]
        yb = fc.bucketed_step(model, dense, axis, x, ids, frames, softmax)
        rec = dict(kind="grouped", id=case["id"], call=ci, path=path, ntiles=ntiles, records=recs, rows=[], y_shape=list(y.shape),
                   read_shape=list(after[0].shape), warm_nonzero=all(bool(c.abs().max() > 0) for c in before) if ci == 0 else True)
        for b, (s, n) in enumerate(zip(ids, frames)):
            if n <= 0:
                rec["rows"].append(dict(row=b, stream=s, frames=n, y_untouched=bool((y[b] == SENTINEL).all()),
                                        cache_kept=bits_equal(after[s], before[s])))
                continue
            got = y[b, :n] if per_frame else y[b]
            ry, ocache[s] = kws_oracle.forward(cfg, sd, x[b:b + 1, :n].cpu().numpy(), ocache[s], softmax=softmax, dtype=np.float64)
            ey, ec = H.tight_error(got.cpu().numpy()[None], ry, yax), H.tight_error(after[s].cpu().numpy(), ocache[s], cax)
            rec["rows"].append(dict(
                row=b, stream=s, frames=n, y_err=ey, cache_err=ec, y_bucketed=bits_equal(got, yb[b]),
                cache_bucketed=bits_equal(after[s], dense.select(axis, s).unsqueeze(axis)),
                tail_untouched=bool((y[b, n:] == SENTINEL).all()) if per_frame else True))
        rec["left_out_kept"] = all(bits_equal(after[s], before[s]) for s in range(S) if s not in ids)
        if ci >= 0:
            emit(**rec)


# ---------------------------------------------------------------------------------------------------------------------------------
def pool_cases(lib, name):
    """d. The pool's own mechanics, each on a pool and on a twin that synchronises after every call: y and every stream's cache bit
    for bit.  ds_tcn_h256 is table-driven, mdtc_h64 takes the grouped path (the scratch)."""
    cfg, sd, model = fc.build(name)
    S, idim, odim = fm.STREAMS, cfg["input_dim"], model.odim
    axis = fc.cache_axis(cfg)
    rng = np.random.default_rng(5)
    rec = dict(kind="pool", model=name)

    def play(calls, sync, pool=None):
        p = pool or StreamCachePool(model, S)
        ys, paths = [], []
        for ids, fr, x in calls:
            y = torch.full((len(ids), x.size(1), odim), SENTINEL, device="cuda")
            model.forward_streams(x, fr, ids, p, out=y)
            paths.append(trace(lib)[:2])
            if sync:
                torch.cuda.synchronize()
            ys.append(y)
        torch.cuda.synchronize()
        return p, ys, paths

    def same(a, b):
        (pa, ya, _), (pb, yb, _) = a, b
        return all(bits_equal(u, v) for u, v in zip(ya, yb)) and all(bits_equal(pa.read(s), pb.read(s)) for s in range(S))

    # nine calls back to back: the ring of four row tables wraps twice
    ring = []
    for k in range(9):
        fr = [int(v) for v in rng.integers(-1, 17, size=5)]
        fr[k % 5] = max(fr[k % 5], 1 + k)
        ring.append(([int(v) for v in rng.permutation(S)[:5]], fr, feats(5, 16, idim, 100 + k)))
    torch.cuda.synchronize()
    a, b = play(ring, False), play(ring, True)
    rec["ring"] = dict(calls=len(ring), same=same(a, b), distinct_ids=len({tuple(c[0]) for c in ring}), distinct_frames=len({tuple(c[1]) for c in ring}))
    # small, more and longer rows, small: the grouped scratch grows between calls that nobody waited for
    grow = [([5, 1], [2, 4], feats(2, 4, idim, 120)), ([0, 1, 2, 3, 4, 6], [16, 9, 16, 3, 12, 16], feats(6, 16, idim, 121)),
            ([1, 5], [1, 3], feats(2, 4, idim, 122))]
    torch.cuda.synchronize()
    a, b = play(grow, False), play(grow, True)
    rec["grow"] = dict(same=same(a, b), paths=a[2])
    # the bucketed step agrees with the growing calls too (not only the twin)
    dense = torch.zeros(pack.cache_shape(model._d, S), dtype=torch.float32, device="cuda")
    ok = True
    for (ids, fr, x), y in zip(grow, a[1]):
        yb = fc.bucketed_step(model, dense, axis, x, ids, fr, False)
        ok = ok and all(bits_equal(y[r, :n], yb[r]) for r, n in enumerate(fr) if n > 0)
    rec["grow"]["bucketed"] = ok and all(bits_equal(a[0].read(s), dense.select(axis, s).unsqueeze(axis)) for s in range(S))
    # write then read gives the bits written, after 0, 1 and 2 steps of the stream (either parity); write then a step = forward alone
    s = 3
    c = torch.from_numpy((0.5 * np.random.default_rng(6).standard_normal(pack.cache_shape(model._d, 1))).astype(np.float32)).cuda()
    x1 = feats(1, 16, idim, 130)
    rec["write_read"], rec["write_step"] = [], []
    for steps in (0, 1, 2):
        p = StreamCachePool(model, S)
        for k in range(steps):
            model.forward_streams(feats(2, 16, idim, 131 + k), [5, 6], [s, 0], p)
        p.write(s, c)
        rec["write_read"].append(bits_equal(p.read(s), c))
        y = torch.full((1, 16, odim), SENTINEL, device="cuda")
        model.forward_streams(x1, [7], [s], p, out=y)
        ya, ca = model.forward(x1[:, :7].contiguous(), c)
        torch.cuda.synchronize()
        rec["write_step"].append(bits_equal(y[0, :7], ya[0]) and bits_equal(p.read(s), ca) and bool((y[0, 7:] == SENTINEL).all()))
    # reset(None) with streams at mixed parity; then ONE call holding all max_streams streams equals that call on a fresh pool
    p = StreamCachePool(model, S)
    model.forward_streams(feats(4, 16, idim, 140), [5, 16, 1, 9], [0, 1, 2, 3], p)
    model.forward_streams(feats(3, 16, idim, 141), [2, 16, 7], [2, 3, 4], p)       # 0, 1, 4: one step; 2, 3: two; 5, 6: none
    nonzero = [bool(p.read(k).abs().max() > 0) for k in range(S)]
    p.reset(None)
    zero = all(bool((p.read(k) == 0).all()) for k in range(S))
    every = [([int(v) for v in rng.permutation(S)], [16, 3, 1, 9, 16, 12, 7], feats(S, 16, idim, 142))]
    a, b = play(every, False, pool=p), play(every, True)
    dense.zero_()
    yb = fc.bucketed_step(model, dense, axis, every[0][2], every[0][0], every[0][1], False)
    rec["reset_all"] = dict(stepped=nonzero, zero=zero, next_call_same=same(a, b), rows=S,
                            bucketed=all(bits_equal(a[1][0][r, :n], yb[r]) for r, n in enumerate(every[0][1])) and
                            all(bits_equal(a[0].read(k), dense.select(axis, k).unsqueeze(axis)) for k in range(S)))
    # refusals: EINVAL, nothing launched, nothing moved
    pool, twin = a[0], b[0]
    L = _capi.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    xr = feats(S + 1, 16, idim, 150)
    y = torch.full((S + 1, 16, odim), SENTINEL, device="cuda")
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)     # noqa: E731
    rec["refusals"] = {}
    for what, (nb, tcap) in {"B > max_streams": (S + 1, 16), "Tcap = 0": (5, 0)}.items():
        ia, fa = i32(list(range(nb))), i32([min(4, tcap)] * nb)
        rc = L.wekws_hip_forward_streams(model._get_handle(xr.device).ptr, pool._ptr, xr.data_ptr(), nb, tcap, ia.ctypes.data, fa.ctypes.data,
                                         y.data_ptr(), 0, stream)
        rec["refusals"][what] = dict(rc=rc, message=_capi.last_error())
    torch.cuda.synchronize()
    handle_before = model._get_handle(xr.device)
    model.set_precision("f16" if name == "ds_tcn_h256" else "f32")
    try:
        model.forward_streams(xr[:5], [4] * 5, list(range(5)), pool, out=y[:5])
        raised = "no error"
    except RuntimeError as e:
        raised = "RuntimeError: " + str(e)[:60]
    torch.cuda.synchronize()
    rec["refusals"]["set_precision"] = dict(raised=raised, handle_changed=model._get_handle(xr.device) is not handle_before)
    rec["refusals"]["y_untouched"] = bool((y == SENTINEL).all())
    rec["refusals"]["streams_untouched"] = all(bits_equal(pool.read(k), twin.read(k)) for k in range(S))
    emit(**rec)


# ---------------------------------------------------------------------------------------------------------------------------------
def nonfinite_case(lib, case):
    """e. Two rows per workgroup: a NaN feature in one row, a +Inf in the carried cache of another row's stream.  The poisoned rows
    AND their slot-mates (the whole workgroup takes the non-finite path) against the oracle's classes and values; every row of
    another workgroup bit-identical to the clean call on a twin pool."""
    cfg, sd, model = build_case(case)
    ids, frames = fm.nonfinite_frames(case, cus())
    B, Tcap = len(ids), case["Tcap"]
    yax, cax = H.y_axis(cfg, False), H.cache_axis(cfg)
    p = fm.plan(lib, cfg, Tcap, frames, cus())
    group_of = {b: g for g, (_, rows) in enumerate(p["groups"]) for b in rows}
    top = max(frames)
    b_nan = next(b for b in range(B) if 2 < frames[b] < top and len(p["groups"][group_of[b]][1]) == 2)
    b_inf = next(b for b in range(B) if frames[b] == top and len(p["groups"][group_of[b]][1]) == 2)
    touched = sorted(set(p["groups"][group_of[b_nan]][1]) | set(p["groups"][group_of[b_inf]][1]))
    xw, x = feats(B, 3, cfg["input_dim"], 21), feats(B, Tcap, cfg["input_dim"], 22)
    xp = x.clone()
    xp[b_nan, 2, 5] = float("nan")
    out = {}
    for tag, xin in (("clean", x), ("poison", xp)):
        pool = StreamCachePool(model, B)
        model.forward_streams(xw, [3] * B, ids, pool)
        if tag == "poison":
            c = pool.read(ids[b_inf])
            c.view(-1)[c.numel() // 3] = float("inf")
            pool.write(ids[b_inf], c)
        cin = torch.cat([pool.read(s) for s in ids], 0)
        y = torch.full((B, Tcap, model.odim), SENTINEL, device="cuda")
        model.forward_streams(xin, frames, ids, pool, out=y)
        torch.cuda.synchronize()
        tr = trace(lib)
        out[tag] = (y, torch.cat([pool.read(s) for s in ids], 0), cin, tr)
    (yc, cc, _, _), (yp, cp, cin, tr) = out["clean"], out["poison"]
    rec = dict(kind="nonfinite_packed", id=case["id"], B=B, path=tr[0], records=tr[2], nan_row=b_nan, inf_row=b_inf, touched=[],
               groups=[p["groups"][group_of[b_nan]][1], p["groups"][group_of[b_inf]][1]])
    for b in touched:
        n = frames[b]
        with np.errstate(all="ignore"):
            ry, rc = kws_oracle.forward(cfg, sd, xp[b:b + 1, :n].cpu().numpy(), cin[b:b + 1].cpu().numpy(), softmax=False, dtype=np.float64)
        rec["touched"].append(dict(row=b, frames=n, poisoned=b in (b_nan, b_inf),
                                   y_err=H.masked_tight_error(yp[b:b + 1, :n].cpu().numpy(), ry, yax),
                                   cache_err=H.masked_tight_error(cp[b:b + 1].cpu().numpy(), rc, cax),
                                   nonfinite=int((~np.isfinite(ry)).sum() + (~np.isfinite(rc)).sum()),
                                   tail_untouched=bool((yp[b, n:] == SENTINEL).all()),
                                   same_as_clean=bits_equal(yp[b], yc[b]) and bits_equal(cp[b], cc[b])))
    others = torch.tensor([b for b in range(B) if b not in touched], device="cuda")
    rec["others"] = int(others.numel())
    rec["others_identical"] = bits_equal(yp.index_select(0, others), yc.index_select(0, others)) and \
        bits_equal(cp.index_select(0, others), cc.index_select(0, others))
    emit(**rec)


SECTIONS = {"fsmn": (fsmn_case, fm.FSMN_CASES), "ds256": (ds256_case, fm.DS256_CASES), "grouped": (grouped_case, fm.GROUPED_CASES),
            "pool": (pool_cases, ["ds_tcn_h256", "mdtc_h64"]), "nonfinite": (nonfinite_case, fm.NONFINITE_CASES)}


def main():
    lib = fm.type_plan(_capi.load())
    assert _capi.lib_path().endswith("libwekws_hip_hooks.so"), _capi.lib_path()
    for section in sys.argv[1:] or list(SECTIONS):
        run, cases = SECTIONS[section]
        t0 = time.time()
        for case in cases:
            run(lib, case)
        torch.cuda.synchronize()
        emit(kind="seconds", section=section, seconds=round(time.time() - t0, 2))
    print("OK")


if __name__ == "__main__":
    main()
