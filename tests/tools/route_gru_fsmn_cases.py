"""Runs the GRU and FSMN calls of the route tests on the GPU with the TEST build of the library (libwekws_hip_hooks.so, for
wekws_hip_debug_route_trace), for tests/test_hip_route_gru_fsmn.py.  Run as a subprocess with WEKWS_HIP_LIB pointing at it:

    python tests/tools/route_gru_fsmn_cases.py [OUT.jsonl [row id ...]]

First the recipe calls of tests/route_matrix.py (GRU_CALLS, FSMN_CALLS): one JSON line per call on stdout, the trace's path and
records.  Then, with OUT.jsonl, every row of tests/route_matrix_rnn.py chunk by chunk, the state / cache carried and the offsets
applied: the trace of every chunk against the prediction, every chunk's output and the state after every chunk against the float64
oracle under the tight bar (tests/helpers.py).  The rows of control_rows() run once more with the one weight matrix that is least
visible on the CPU rounded to fp16, against the oracle of the UNROUNDED weights (the negative control: a lost lo(w) term must
miss the bar).  One JSON record per run; then OK: exit code 0 when every run was MADE (the parent asserts on the records)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import route_matrix as rm  # noqa: E402
from tests import route_matrix_rnn as rr  # noqa: E402
from wekws_amd import _capi, pack  # noqa: E402
from wekws_amd.model.kws_model import init_model  # noqa: E402
from wekws_amd.utils import synth  # noqa: E402

MAX = 8


def trace(lib):
    out = (ctypes.c_int * (2 + 9 * MAX))()
    n = lib.wekws_hip_debug_route_trace(out, MAX)
    return out[0], out[1], [list(out[2 + 9 * i:11 + 9 * i]) for i in range(n)]


def offset_copy(t, off):
    """A contiguous copy of t that starts `off` floats into a larger allocation (pointers only 4-byte aligned for off % 4)."""
    if not off:
        return t.contiguous()
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * (off % 4)
    return v


def build(cfg, sd, row=None):
    m = init_model(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.cuda().eval()
    if row is not None:
        m.set_precision(row["precision"])
        for k, v in row["opts"].items():
            m.set_option(k, v)
    return m


def recipe_calls(lib, cus):
    models = {}
    for name, B, T in rm.GRU_CALLS + rm.FSMN_CALLS:
        cfg = synth.MODEL_CONFIGS[name]
        if name not in models:
            models[name] = build(cfg, synth.synth_state_dict(pack.model_spec(cfg), 1234))
        x = torch.from_numpy(synth.synth_feats(B, T, cfg["input_dim"], seed=3)).cuda()
        models[name](x)
        torch.cuda.synchronize()
        path, ntiles, recs = trace(lib)
        print(json.dumps(dict(model=name, B=B, T=T, cus=cus, path=path, ntiles=ntiles, records=recs)), flush=True)


def run_row(lib, row, cfg, sd, x, s0, refs, matrix=None):
    """One run of the row with weights sd (matrix: the one rounded to fp16, for the record) against the references refs."""
    model = build(cfg, sd, row)
    plan, expect = rr.EXPECT[row["id"]]
    xt = torch.from_numpy(x).cuda()
    c = None if s0 is None else torch.from_numpy(s0).cuda()
    ys, cs, got, paths, t = [], [], [], [], 0
    for n in row["chunks"]:
        xc = offset_copy(xt[:, t:t + n], row["x_off"])
        cin = None if c is None else offset_copy(c, row["c_off"])
        y, c = model(xc) if cin is None else model(xc, cin)
        torch.cuda.synchronize()
        path, ntiles, recs = trace(lib)
        paths.append(path)
        if ntiles != len(recs):
            recs = recs + ["?"] * (ntiles - len(recs))
        if row["kind"] == "gru" and plan != "generic":
            recs = [rm.GRU_FAMILIES[recs[0][0]]] + recs[0][1:] if len(recs) == 1 else ["?"] + recs
        got.append(recs)
        ys.append(y.cpu().numpy())
        cs.append(c.cpu().numpy())
        t += n
    want_path = 2 if plan == "generic" else 3 if row["kind"] == "gru" else 4
    ey, ec = rr.row_errors(cfg, ys, cs, *refs, row["stream_scale"])
    return dict(id=row["id"], control=matrix is not None, matrix=matrix, plan=plan, expect=expect, got=got, paths=paths,
                trace_ok=(got == expect) and all(p == want_path for p in paths), y_err=ey, state_err=ec,
                chunk_err=rr.chunk_errors(row, cfg, ys, cs, *refs), err=rr.row_error(row, cfg, ys, cs, *refs))


def main():
    lib = rm.type_hooks(_capi.load())
    assert _capi.lib_path().endswith("libwekws_hip_hooks.so"), _capi.lib_path()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    recipe_calls(lib, cus)
    if len(sys.argv) > 1:
        assert cus == rr.CUS, f"the route matrix predicts for {rr.CUS} compute units; this device has {cus}"
        only = sys.argv[2:]
        control = {r["id"] for r in rr.control_rows()}
        with open(sys.argv[1], "w") as f:
            for row in rr.ROWS:
                if only and row["id"] not in only:
                    continue
                cfg = rr.row_config(row)
                sd = rr.row_weights(row, cfg)
                x, s0 = rr.row_input(row, cfg), rr.row_state(row, cfg)
                refs = rr.reference(cfg, sd, x, s0, row["chunks"], np.float64)
                f.write(json.dumps(run_row(lib, row, cfg, sd, x, s0, refs)) + "\n")
                f.flush()
                if row["id"] in control:
                    # (the choice is a CPU fact -- the float32 oracle at <= 4 utterances, a fraction of a second per row --, made
                    # here and not kept as a literal: two matrices of a row can be within a percent of each other)
                    name = rr.least_visible_matrix(row)
                    f.write(json.dumps(run_row(lib, row, cfg, rr.rounded(sd, name), x, s0, refs, matrix=name)) + "\n")
                    f.flush()
    print("OK")


if __name__ == "__main__":
    main()
