"""Runs every row of tests/route_matrix.py on the GPU with the TEST build of the library (libwekws_hip_hooks.so, for its tile trace
wekws_hip_debug_route_trace), for tests/test_hip_route_matrix.py.  Run as a subprocess with WEKWS_HIP_LIB pointing at it:

    python tests/tools/route_matrix_cases.py OUT.jsonl

Per row, chunk by chunk with the cache carried: the tile trace of the forward against the prediction, and each chunk's output and
the final cache against the float64 oracle under the tight bar (tests/helpers.py).  Every F16X3 row runs once more with
set_precision("f16") (the negative control: one fp16 product must miss the bar).  One JSON record per run; exit code 0 when every
run was MADE (the parent asserts on the records)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import route_matrix as rm  # noqa: E402
from tests.helpers import cache_axis, oracle64, tight_error, y_axis  # noqa: E402
from wekws_amd import _capi  # noqa: E402
from wekws_amd.model.kws_model import init_model  # noqa: E402

MAX_TILES = 8


def trace(lib, B):
    out = (ctypes.c_int * (2 + 9 * MAX_TILES))()
    n = lib.wekws_hip_debug_route_trace(out, MAX_TILES)
    path, ntiles = out[0], out[1]
    tiles = [rm.route_str(dict(zip(rm.TRACE_KEYS, out[2 + 9 * i:11 + 9 * i]), family=rm.FAMILIES[out[2 + 9 * i]]), B) for i in range(n)]
    return path, ntiles, tiles


def offset_copy(t, off):
    """A contiguous copy of t that starts `off` floats into a larger allocation (pointers only 4-byte aligned for off % 4)."""
    if not off:
        return t.contiguous()
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * (off % 4)
    return v


def run_row(lib, row, precision):
    cfg = rm.row_config(row)
    cfg["_precision"] = precision
    sd = rm.row_weights(row, cfg)
    x = rm.row_input(row, cfg)
    c0 = rm.row_cache(row, cfg)
    model = init_model(cfg)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.cuda().eval().set_precision(precision)
    for k, v in row["opts"].items():
        model.set_option(k, v)
    plan, expect = rm.EXPECT[row["id"]] if precision == row["precision"] else rm.predict(lib, row, precision)
    xt = torch.from_numpy(x).cuda()
    c = None if c0 is None else torch.from_numpy(c0).cuda()
    ys, got, paths, t = [], [], [], 0
    for n in row["chunks"]:
        xc = offset_copy(xt[:, t:t + n], row["x_off"])
        cin = None if c is None else offset_copy(c, row["c_off"])
        y, c = model(xc) if cin is None else model(xc, cin)
        torch.cuda.synchronize()
        path, ntiles, tiles = trace(lib, row["B"])
        paths.append(path)
        got.append(tiles if ntiles == len(tiles) else tiles + ["?"] * (ntiles - len(tiles)))
        ys.append(y.cpu().numpy())
        t += n
    ry, rc = oracle64(cfg, sd, x, c0, row["chunks"])
    errs, t = [], 0
    for j, n in enumerate(row["chunks"]):
        ry_j = ry[:, t:t + n] if ry.ndim == 3 else ry[:, j * cfg["output_dim"]:(j + 1) * cfg["output_dim"]]
        errs.append(tight_error(ys[j], ry_j, y_axis(cfg)))
        t += n
    ec = tight_error(c.cpu().numpy(), rc, cache_axis(cfg))
    want_path = 2 if plan == "generic" else 1
    return dict(id=row["id"], precision=precision, plan=plan, expect=expect, got=got, paths=paths, path_ok=all(p == want_path for p in paths),
                trace_ok=(got == expect) and all(p == want_path for p in paths), y_err=errs, cache_err=ec, err=max(errs + [ec]))


def main():
    out = sys.argv[1]
    lib = rm.type_hooks(_capi.load())
    assert _capi.lib_path().endswith("libwekws_hip_hooks.so"), _capi.lib_path()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == rm.CUS, f"the route matrix predicts for {rm.CUS} compute units; this device has {cus}"
    only = sys.argv[2:]
    with open(out, "w") as f:
        for row in rm.ROWS:
            if only and row["id"] not in only:
                continue
            f.write(json.dumps(run_row(lib, row, row["precision"])) + "\n")
            f.flush()
            if rm.is_split_row(row):
                f.write(json.dumps(dict(run_row(lib, row, "f16"), control=True)) + "\n")
                f.flush()
    print("OK")


if __name__ == "__main__":
    main()
