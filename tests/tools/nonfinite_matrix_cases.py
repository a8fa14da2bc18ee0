"""Runs the poisoned matrix (tests/nonfinite_matrix.py) and the named non-finite stress rows on the GPU with the TEST build of the
library (libwekws_hip_hooks.so, for wekws_hip_debug_route_trace), for tests/test_hip_nonfinite_matrix.py.  Run as a subprocess
with WEKWS_HIP_LIB pointing at it:

    python tests/tools/nonfinite_matrix_cases.py matrix OUT.jsonl [row id ...]
    python tests/tools/nonfinite_matrix_cases.py stress NAME OUT.jsonl

matrix: every derived row chunk by chunk with the cache / state carried and the offsets applied -- the trace of every chunk
against the base row's prediction, the classes (finite / NaN / +Inf / -Inf) of every chunk's output and of the state after every
chunk against the float64 oracle, and the masked tight error (tests/helpers.py::masked_tight_error) separately over
  * "repaired": a poisoned utterance in a call whose features or incoming cache / state are non-finite (the IEEE f32 repair
    ran: held to TIGHT_K under every precision; under f16 only while every earlier call of the utterance was repaired too), and
  * "clean": everything else (TIGHT_K; under precision f16 the fast path's own bar, 2e-2 max(1, max|ref|), in units of it);
rows all of whose tiles run a one-utterance-per-workgroup DS-TCN h256 kernel also run WITHOUT the poison, and their clean
utterances are compared with that run bit for bit.
stress: one named row (STRESS) -- shapes that overflow the persistent kernels' list of noted utterances, or hold more poisoned
workgroups than the model has scratch slots.  One JSON record per run; then OK: exit code 0 when every run was MADE (the parent
asserts on the records)."""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import nonfinite_matrix as nm  # noqa: E402
from tests import route_matrix as rm  # noqa: E402
from tests.helpers import cache_axis, masked_tight_error, value_classes, y_axis  # noqa: E402
from wekws_amd import _capi  # noqa: E402
from wekws_amd.model.kws_model import init_model  # noqa: E402
from wekws_amd.utils import synth  # noqa: E402

MAX = 8
F16_CLEAN = 2e-2                  # the fast path's bar under precision f16 (tests/test_hip_nonfinite.py)


def trace(lib, kind, B, plan):
    """The trace of the last forward in the form of the matrices' EXPECT tables."""
    out = (ctypes.c_int * (2 + 9 * MAX))()
    n = lib.wekws_hip_debug_route_trace(out, MAX)
    path, ntiles = out[0], out[1]
    recs = [list(out[2 + 9 * i:11 + 9 * i]) for i in range(n)]
    if kind == "conv":
        got = [rm.route_str(dict(zip(rm.TRACE_KEYS, r), family=rm.FAMILIES[r[0]]), B) for r in recs]
    elif kind == "gru" and plan != "generic":
        got = [rm.GRU_FAMILIES[recs[0][0]]] + recs[0][1:] if len(recs) == 1 else ["?"] + recs
        return path, got
    else:
        got = recs
    return path, got + ["?"] * (ntiles - len(got))


def offset_copy(t, off):
    """A contiguous copy of t that starts `off` floats into a larger allocation (pointers only 4-byte aligned for off % 4)."""
    if not off:
        return t.contiguous()
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * (off % 4)
    return v


def build(cfg, sd, precision, opts):
    m = init_model(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.cuda().eval().set_precision(precision)
    for k, v in opts.items():
        m.set_option(k, v)
    return m


def forward(lib, model, kind, plan, B, x, c0, chunks, x_off=0, c_off=0):
    """-> ([y of every chunk], [state after every chunk], [trace of every chunk], [path of every chunk])."""
    xt = torch.from_numpy(x).cuda()
    c = None if c0 is None else torch.from_numpy(c0).cuda()
    ys, cs, got, paths, t = [], [], [], [], 0
    for n in chunks:
        xc = offset_copy(xt[:, t:t + n], x_off)
        cin = None if c is None else offset_copy(c, c_off)
        y, c = model(xc) if cin is None else model(xc, cin)
        torch.cuda.synchronize()
        path, recs = trace(lib, kind, B, plan)
        paths.append(path)
        got.append(recs)
        ys.append(y.cpu().numpy())
        cs.append(c.cpu().numpy())
        t += n
    return ys, cs, got, paths


def bad_inputs(kind, x, incoming, a, b, utts):
    """Of the utterances utts: those whose features in the frames [a, b) or whose incoming cache / state are non-finite."""
    out = []
    for u in utts:
        xb = not np.isfinite(x[u, a:b]).all()
        cb = incoming is not None and not np.isfinite(nm.take(kind, incoming, [u])).all()
        if xb or cb:
            out.append(u)
    return out


def compare(kind, cfg, precision, x, c0, chunks, ys, cs, rys, rcs, bad, stream_scale=False):
    """(classes equal everywhere, error of the repaired part in units of TIGHT_K's scale, error of the clean part [under f16: in
    units of its own bar], per chunk)."""
    scale = np.concatenate(rys, axis=1) if stream_scale else None
    B = x.shape[0]
    class_ok, e_bad, e_clean, t = True, [], [], 0
    exact = set(bad)
    for j, n in enumerate(chunks):
        incoming = c0 if j == 0 else rcs[j - 1]
        rep = bad_inputs(kind, x, incoming, t, t + n, bad)
        if precision == "f16":        # behind a fast-path call the repair starts from a cache of fp16 precision: exact only from the start
            exact &= set(rep)
            rep = sorted(exact)
        rest = [u for u in range(B) if u not in rep]
        y, ry, c, rc = ys[j], rys[j], cs[j], rcs[j]
        class_ok &= bool(np.array_equal(value_classes(y), value_classes(ry)) and np.array_equal(value_classes(c), value_classes(rc)))
        my, mc = nm.utt_mask(kind, ry.shape, rep), nm.utt_mask(kind, rc.shape, rep, state=True)
        e_bad.append(max(masked_tight_error(y, ry, y_axis(cfg), my, scale), masked_tight_error(c, rc, cache_axis(cfg), mc)))
        my, mc = nm.utt_mask(kind, ry.shape, rest), nm.utt_mask(kind, rc.shape, rest, state=True)
        if precision == "f16":
            e = 0.0
            for g, r, m in ((y, ry, my), (c, rc, mc)):
                fin = np.isfinite(r) & m
                if not np.array_equal(value_classes(g)[m], value_classes(r)[m]):
                    e = float("inf")
                elif fin.any():
                    e = max(e, float(np.abs(g[fin].astype(np.float64) - r[fin]).max()) / (F16_CLEAN * max(1.0, float(np.abs(r[fin]).max()))))
            e_clean.append(e)
        else:
            e_clean.append(max(masked_tight_error(y, ry, y_axis(cfg), my, scale), masked_tight_error(c, rc, cache_axis(cfg), mc)))
        t += n
    return class_ok, e_bad, e_clean


def one_per_workgroup_h256(expect):
    tiles = [t for ch in expect for t in ch]
    return bool(tiles) and all(isinstance(t, str) and t.startswith("ds256") and " upw1 " in t for t in tiles)


def run_row(lib, row):
    base, kind = row["base"], row["kind"]
    cfg, sd, x, c, x0, c0 = nm.row_case(row)
    plan, expect = nm.expect(row, lib)
    model = build(cfg, sd, row["precision"], base["opts"])
    B, chunks = base["B"], base["chunks"]
    ys, cs, got, paths = forward(lib, model, kind, plan, B, x, c, chunks, base["x_off"], base["c_off"])
    want_path = 2 if plan == "generic" else {"conv": 1, "gru": 3, "fsmn": 4}[kind]
    bitwise = None
    clean = [u for u in range(B) if u not in row["bad"]]
    pick = list(range(B))
    if kind == "conv" and plan != "generic" and one_per_workgroup_h256(expect) and clean:
        yc, cc, _, _ = forward(lib, model, kind, plan, B, x0, c0, chunks, base["x_off"], base["c_off"])
        bitwise = all(np.array_equal(a[clean], b[clean]) for a, b in zip(ys + cs, yc + cc))
        if B > 16:
            # a large batch whose clean utterances ARE the clean call's (which tests/test_hip_route_matrix.py holds to the oracle at
            # the full batch): the oracle on the poisoned utterances, their neighbours and the first clean ones -- 12 in all
            near = [u for b in row["bad"] for u in (b - 1, b + 1) if u in set(clean)]
            pick = sorted(set(row["bad"]) | set((near + clean)[:12 - len(row["bad"])]))
    sub = lambda a: None if a is None else np.ascontiguousarray(a[pick])                  # noqa: E731  (conv: the batch axis is the first)
    if len(pick) < B:
        x, c, ys, cs = sub(x), sub(c), [sub(y) for y in ys], [sub(a) for a in cs]
    bad = [pick.index(u) for u in row["bad"]]
    rys, rcs = nm.reference(cfg, sd, x, c, chunks, np.float64)
    class_ok, e_bad, e_clean = compare(kind, cfg, row["precision"], x, c, chunks, ys, cs, rys, rcs, bad, base.get("stream_scale", False))
    segs = nm.segments(base)
    keys = sorted({nm.tuple_key(kind, segs[s][3]) for s, _, _ in row["claims"]})
    return dict(id=row["id"], precision=row["precision"], plan=plan, expect=expect, got=got, paths=paths,
                trace_ok=(got == expect) and all(p == want_path for p in paths), class_ok=class_ok, err_repaired=e_bad, err_clean=e_clean,
                bitwise=bitwise, keys=keys, nbad=len(row["bad"]), noracle=len(pick))


# ---------------------------------------------------------------------------------------------------------------------------------
# the named stress rows
def _model(name, over=None):
    import copy
    cfg = copy.deepcopy(synth.MODEL_CONFIGS[name])
    cfg.update(over or {})
    return cfg


def _poison(x, utts, frame, feature=3):
    for k, u in enumerate(utts):
        x[u, frame, (feature + k) % x.shape[2]] = nm.VALUES[k % 5]


# name -> (model, config overrides, precision, options, B, chunks, poisoned utterances, frame of the poison, repeats)
# B = 7681 on 256 persistent workgroups: workgroup g walks b = g, g + 256, ...  Every step of workgroup 0's walk (31: one more than
# the list of noted utterances holds, the re-scan), every step of workgroup 1's (30: the full list), and EVERY OTHER step of
# workgroup 2's (15 of 30): there a noted utterance is followed by a clean one on the fast path and a clean one by a noted one.
NFLIST = sorted(set(range(0, 7681, 256)) | set(range(1, 7681, 256)) | set(range(2, 7681, 512)))
FORTY = [u for u in range(64) if u % 8 not in (2, 5, 7)]                     # 40 of 64: pairs, runs and single clean neighbours
STRESS = {
    # the persistent kernels note at most 30 poisoned utterances per workgroup: 31 (the re-scan), exactly 30 (the full list) and a
    # walk that alternates; in the second chunk (the context variant) the poison arrives through the carried cache alone
    "nflist_g16": ("ds_tcn_h256", {}, "default", {}, 7681, (17, 17), NFLIST, 16, 1),
    "nflist_g32": ("ds_tcn_h256", {}, "f32", {}, 7681, (17,), NFLIST, 16, 1),
    # more poisoned workgroups than the 16 scratch slots, twice on one model (slots are taken again with stale contents)
    "slots_conv_upw1": ("ds_tcn_h256", {}, "default", {}, 64, (40,), FORTY, 20, 2),
    "slots_conv_upw2": ("tcn_h64", {}, "default", {}, 64, (40,), FORTY, 20, 2),
    "slots_gru_fix": ("gru_2x128", {"output_dim": 40, "activation": {"type": "identity"}}, "default", {"gru_pipe": 0}, 64, (10,), FORTY, 5, 2),
    "slots_fsmn": ("fsmn_small", {"output_dim": 13}, "default", {}, 64, (20,), FORTY, 10, 2),
}


def stress_predict(lib, name):
    """The routes route.h chooses for the row's calls: (kind, plan, per chunk the trace in the matrices' form)."""
    model, over, precision, opts, B, chunks, _, _, _ = STRESS[name]
    cfg = _model(model, over)
    kind = {"tcn": "conv", "mdtc": "conv"}.get(cfg["backbone"]["type"], cfg["backbone"]["type"])
    row = dict(id=name, kind=kind, model=model, over=over, precision=precision, opts=opts, B=B, chunks=list(chunks), cache=False, state=None,
               x_off=0, c_off=0)
    if kind == "conv":
        plan, expect = _conv_predict(lib, row, cfg)
    else:
        plan, expect = _rnn_predict(lib, row, cfg)
    return kind, plan, expect


def _conv_predict(lib, row, cfg):
    import math
    out = []
    for j, T in enumerate(row["chunks"]):
        tiles = []
        for i in range(math.ceil(T / rm.TILE)):
            r = rm.route(lib, cfg, row["B"], min(rm.TILE, T - i * rm.TILE), has_in=bool(j or i), has_out=True, precision=row["precision"],
                         ntiles=math.ceil(T / rm.TILE), opts=rm.route_opts(row))
            tiles.append(rm.route_str(r, row["B"]))
        out.append(tiles)
    return "as_is", out


def _rnn_predict(lib, row, cfg):
    out = []
    for T in row["chunks"]:
        if row["kind"] == "gru":
            out.append(rm.gru_record(rm.gru_route(lib, cfg, row["B"], T, precision=row["precision"], opts=row["opts"])))
        else:
            first = rm.fsmn_route(lib, cfg, row["B"], T, precision=row["precision"], opts=row["opts"])
            out.append([rm.fsmn_record(rm.fsmn_route(lib, cfg, row["B"], T, tile=i, precision=row["precision"], opts=row["opts"]))
                        for i in range(first["ntiles"])])
    return "as_is", out


def run_stress(lib, name):
    from wekws_amd import pack
    model_name, over, precision, opts, B, chunks, bad, frame, repeats = STRESS[name]
    cfg = _model(model_name, over)
    cfg["_precision"] = precision
    kind, plan, expect = stress_predict(lib, name)
    sd = synth.synth_state_dict(pack.model_spec(cfg), 4321)
    x0 = synth.synth_feats(B, sum(chunks), cfg["input_dim"], seed=11)
    x = x0.copy()
    _poison(x, bad, frame)
    model = build(cfg, sd, precision, opts)
    # the oracle on every poisoned utterance and on 16 clean ones spread over the batch (the models are per utterance)
    clean = [u for u in range(B) if u not in set(bad)]
    walk2 = [u for u in range(2, B, rm.CUS) if u in set(clean)][:4] if B > rm.CUS else []      # clean steps of a mixed walk
    sample = sorted(set(bad + walk2 + [clean[(i * len(clean)) // 16] for i in range(16)]))
    sbad = [sample.index(u) for u in bad]
    rys, rcs = nm.reference(cfg, sd, x[sample], None, chunks, np.float64)
    recs = []
    for rep in range(repeats):
        t0 = time.time()
        ys, cs, got, paths = forward(lib, model, kind, plan, B, x, None, chunks)
        secs = time.time() - t0
        sub = lambda a, state=False: nm.take(kind, a, sample) if state else a[sample]          # noqa: E731
        class_ok, e_bad, e_clean = compare(kind, cfg, precision, x[sample], None, chunks, [sub(y) for y in ys], [sub(c, True) for c in cs],
                                           rys, rcs, sbad)
        bitwise = None
        if kind == "conv" and one_per_workgroup_h256(expect):
            yc, cc, _, _ = forward(lib, model, kind, plan, B, x0, None, chunks)
            bitwise = all(np.array_equal(a[clean], b[clean]) for a, b in zip(ys + cs, yc + cc))
        # every clean utterance of the batch is finite, every poisoned one is not
        finite_ok = all(np.isfinite(y[clean]).all() for y in ys) and all(not np.isfinite(ys[0][u]).all() for u in bad)
        want_path = {"conv": 1, "gru": 3, "fsmn": 4}[kind]
        recs.append(dict(id=name, repeat=rep, expect=expect, got=got, paths=paths, trace_ok=(got == expect) and all(p == want_path for p in paths),
                         class_ok=class_ok, err_repaired=e_bad, err_clean=e_clean, bitwise=bitwise, finite_ok=bool(finite_ok), seconds=secs,
                         nbad=len(bad), noracle=len(sample)))
    return recs


def main():
    mode, args = sys.argv[1], sys.argv[2:]
    lib = rm.type_hooks(_capi.load())
    assert _capi.lib_path().endswith("libwekws_hip_hooks.so"), _capi.lib_path()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == rm.CUS, f"the route matrices predict for {rm.CUS} compute units; this device has {cus}"
    if mode == "matrix":
        only = args[1:]
        with open(args[0], "w") as f:
            for row in nm.ROWS:
                if only and row["id"] not in only:
                    continue
                t0 = time.time()
                rec = run_row(lib, row)
                rec["seconds"] = time.time() - t0
                f.write(json.dumps(rec) + "\n")
                f.flush()
    else:
        with open(args[1], "w") as f:
            for rec in run_stress(lib, args[0]):
                f.write(json.dumps(rec) + "\n")
                f.flush()
    print("OK")


if __name__ == "__main__":
    main()
