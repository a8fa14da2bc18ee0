"""Runs every row of tests/softmax_matrix.py on the GPU with the TEST build of the library (libwekws_hip_hooks.so:
wekws_hip_debug_softmax_rows, the route trace), for tests/test_hip_softmax_f64.py.  Run as a subprocess with WEKWS_HIP_LIB
pointing at it:

    python tests/tools/softmax_matrix_cases.py OUT.jsonl [row ids]

Per row: softmax_rows_kernel in place on a buffer with two sentinel rows before and after it, softmax_topk_kernel into outputs
with a sentinel row either side; the largest softmax_units figure of each against the float64 oracle (inf: a class mismatch), the
indices against the oracle's, the sentinels bit for bit.  Then the five ties of the hook to the product path: forward(softmax = 1)
against the hook applied to the same call's logits, bit for bit.  One JSON record per row or tie; this process only records -- the
parent asserts -- and nothing is run again after a failure: the first exception ends the process."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import topk_oracle  # noqa: E402
from tests import softmax_matrix as sm  # noqa: E402
from wekws_amd import _capi, pack  # noqa: E402
from wekws_amd.model.kws_model import init_model  # noqa: E402
from wekws_amd.utils import synth  # noqa: E402

SENTINEL = 2                     # sentinel rows either side of the in-place buffer


def type_hooks(lib):
    lib.wekws_hip_debug_softmax_rows.restype = C.c_int
    lib.wekws_hip_debug_softmax_rows.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    lib.wekws_hip_debug_route_trace.restype = C.c_int
    lib.wekws_hip_debug_route_trace.argtypes = [C.POINTER(C.c_int), C.c_int]
    return lib


def bits_equal(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def framed(inner, pad_rows, fill):
    """A device buffer of pad_rows sentinel rows, `inner`, pad_rows sentinel rows -> (buffer, the view of inner's place)."""
    rows, width = inner.shape
    buf = torch.full(((rows + 2 * pad_rows), width), fill, dtype=inner.dtype, device="cuda")
    if inner.dtype == torch.float32:
        buf += torch.arange(buf.numel(), device="cuda", dtype=torch.float32).view(buf.shape) * 0.25
    view = buf[pad_rows:pad_rows + rows]
    view.copy_(inner)
    assert view.is_contiguous()
    return buf, view


def softmax_rows(lib, y):
    """The hook, in place on the contiguous device tensor y (rows, K)."""
    stream = torch.cuda.current_stream().cuda_stream
    _capi.check(lib.wekws_hip_debug_softmax_rows(y.data_ptr(), y.shape[0], y.shape[1], C.c_void_p(stream)), "wekws_hip_debug_softmax_rows")


def worst(u):
    j = np.unravel_index(int(np.argmax(u)), u.shape)
    return float(u[j]), [int(v) for v in j]


def run_row(lib, row):
    x = sm.row_logits(row)
    xt = torch.from_numpy(x)
    rec = dict(id=row.id, law=row.law, K=row.K, rows=row.rows, k=row.k)
    # ---- softmax_rows_kernel, in place between sentinel rows
    buf, view = framed(xt, SENTINEL, 12345.0)
    before = buf.clone()
    softmax_rows(lib, view)
    torch.cuda.synchronize()
    got = view.cpu().numpy()
    rec["rows_sentinels"] = bits_equal(buf[:SENTINEL], before[:SENTINEL]) and bits_equal(buf[-SENTINEL:], before[-SENTINEL:])
    rec["rows_u"], rec["rows_worst"] = worst(topk_oracle.softmax_units(got, x))
    rec["rows_nan"] = int(np.isnan(got).sum())
    # ---- softmax_topk_kernel: logits between sentinel rows too (an odd K leaves the rows dword aligned), outputs framed
    lbuf, lview = framed(xt, SENTINEL, -54321.0)
    lbefore = lbuf.clone()
    pbuf, pview = framed(torch.zeros(row.rows, row.k), 1, 777.0)
    ibuf, iview = framed(torch.zeros(row.rows, row.k, dtype=torch.int32), 1, 424242)
    pbefore, ibefore = pbuf.clone(), ibuf.clone()
    stream = torch.cuda.current_stream().cuda_stream
    _capi.check(lib.wekws_hip_softmax_topk(lview.data_ptr(), row.rows, row.K, row.k, pview.data_ptr(), iview.data_ptr(), C.c_void_p(stream)),
                "wekws_hip_softmax_topk")
    torch.cuda.synchronize()
    gp, gi = pview.cpu().numpy(), iview.cpu().numpy().astype(np.int64)
    rp, ri = topk_oracle.softmax_topk_f64(x, row.k)
    rec["topk_sentinels"] = (bits_equal(lbuf, lbefore) and bits_equal(pbuf[:1], pbefore[:1]) and bits_equal(pbuf[-1:], pbefore[-1:])
                             and bool(torch.equal(ibuf[:1], ibefore[:1])) and bool(torch.equal(ibuf[-1:], ibefore[-1:])))
    rec["topk_idx_in_range"] = bool(((gi >= -1) & (gi < row.K)).all())
    rec["topk_idx_equal"] = bool(np.array_equal(gi, ri))
    rec["topk_u"], rec["topk_worst"] = worst(topk_oracle.softmax_units(gp, x, ri)) if rec["topk_idx_equal"] else (float("inf"), [])
    if not rec["topk_idx_equal"]:
        bad = int(np.flatnonzero((gi != ri).any(axis=1))[0])
        rec["topk_first_mismatch"] = dict(row=bad, got=gi[bad].tolist(), want=ri[bad].tolist(), probs=[float(v) for v in gp[bad]])
    return rec


# The five ties of the hook to the product path (B = 3, T = 5: 15 rows, a partial last workgroup): one model per forward path of
# wekws_hip_forward (the trace's path: 1 conv routes, 2 any-shape, 3 GRU, 4 FSMN) and one whose activation IS the softmax.
def _cfg(name, **kw):
    return dict(synth.MODEL_CONFIGS[name], **kw)


TIES = (("conv_ctc", 1, _cfg("ds_tcn_h256_ctc300"), False),
        ("gru", 3, _cfg("gru_2x128", output_dim=7, activation=dict(type="identity")), False),
        ("fsmn", 4, _cfg("fsmn_ctc300"), False),
        ("any_shape", 2, _cfg("ds_tcn_h64_ctc20", backbone=dict(synth.MODEL_CONFIGS["ds_tcn_h64_ctc20"]["backbone"], kernel_size=9)), False),
        ("exported_softmax", 1, _cfg("ds_tcn_h64_ctc20"), True))


def build(cfg, sd):
    m = init_model(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.cuda().eval()


def trace_path(lib):
    out = (C.c_int * 11)()
    lib.wekws_hip_debug_route_trace(out, 1)
    return int(out[0])


def run_tie(lib, name, path, cfg, exported):
    B, T = 3, 5
    sd = synth.synth_state_dict(pack.model_spec(cfg), 1234)
    x = torch.from_numpy(synth.synth_feats(B, T, cfg["input_dim"], seed=5) * 3.0).cuda()
    plain = build(cfg, sd)
    logits = plain.posteriors(x, softmax=False)
    got_path = trace_path(lib)
    model = build(dict(cfg, _exported_softmax=True), sd) if exported else plain
    soft = model.posteriors(x, softmax=True)
    same_path = trace_path(lib) == got_path
    soft0 = model.posteriors(x, softmax=False) if exported else None       # activation == SOFTMAX: applied whatever the argument says
    hooked = logits.clone()
    softmax_rows(lib, hooked.view(B * T, -1))
    torch.cuda.synchronize()
    lg = logits.cpu().numpy().reshape(B * T, -1)
    return dict(id="tie/" + name, path=got_path, want_path=path, same_path=same_path, rows=B * T, K=int(logits.shape[-1]),
                shape_ok=tuple(logits.shape) == (B, T, cfg["output_dim"]) == tuple(soft.shape),
                equal=bits_equal(soft, hooked), equal_softmax0=None if soft0 is None else bits_equal(soft0, hooked),
                changed=not bits_equal(soft, logits), u=float(topk_oracle.softmax_units(soft.cpu().numpy().reshape(B * T, -1), lg).max()))


def main():
    out = sys.argv[1]
    lib = type_hooks(_capi.load())
    assert _capi.lib_path().endswith("libwekws_hip_hooks.so"), _capi.lib_path()
    only = sys.argv[2:]
    with open(out, "w") as f:
        for row in sm.ROWS:
            if only and row.id not in only:
                continue
            f.write(json.dumps(run_row(lib, row)) + "\n")
            f.flush()
        for tie in TIES:
            if only and "tie/" + tie[0] not in only:
                continue
            f.write(json.dumps(run_tie(lib, *tie)) + "\n")
            f.flush()
    print("OK")


if __name__ == "__main__":
    main()
