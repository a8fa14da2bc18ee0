"""GPU: the route matrix (tests/route_matrix.py) on the device.  A child process with the TEST build of the library
(libwekws_hip_hooks.so: its tile trace) runs every row -- tests/tools/route_matrix_cases.py --, and per row:
  * the route of every tile of every chunk (wekws_hip_debug_route_trace) equals the prediction the CPU suite checks against route.h:
    the test ran the kernel family and variant it is named for, not a neighbour that happens to be green;
  * every chunk's output and the final cache meet the tight bar (tests/helpers.py::TIGHT_K) against the float64 oracle;
  * the negative control: every F16X3 row rerun with set_precision("f16") MISSES the bar where its trace says one fp16 product
    (split 0) -- the comparison can tell one fp16 product from three on the device, not just in the CPU emulation
    (tests/test_route.py) --, and still MEETS it where the family has no such variant (ds256_mm, dense_stack_f16, conv_stack_f16
    run three products whatever is asked; route.h reports split 1 for them).
The measured error per (family, variant) goes to the session's error report (tests/conftest.py::error_report)."""
import json
import os
import subprocess
import sys

import pytest

from tests import route_matrix as rm
from tests.helpers import TIGHT_K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "tools", "route_matrix_cases.py")


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    hooks = rm.hooks_path()
    assert os.path.exists(hooks), f"{hooks} is missing: make -C wekws_amd/csrc hooks (or __graft_entry__.build())"
    out = str(tmp_path_factory.mktemp("route_matrix") / "records.jsonl")
    env = dict(os.environ, WEKWS_HIP_LIB=hooks)
    r = subprocess.run([sys.executable, CASES, out], env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    recs = {}
    with open(out) as f:
        for line in f:
            d = json.loads(line)
            recs[(d["id"], bool(d.get("control")))] = d
    return recs


def _report(error_report, d):
    for ch in d["got"]:
        for t in ch:
            f, nt, ctx, fast, pers, upw, split = t.split()
            key = f"route_matrix/{'f16_control/' if d.get('control') else ''}{f}/{nt}_{ctx}_{fast}_{pers}_{split}"
            error_report[key] = max(error_report.get(key, 0.0), d["err"])


@pytest.mark.parametrize("row", rm.ROWS, ids=[r["id"] for r in rm.ROWS])
def test_route_matrix_row(row, records, error_report):
    d = records[(row["id"], False)]
    _report(error_report, d)
    assert d["trace_ok"], ("tile routes", d["expect"], d["got"], d["paths"])
    assert d["err"] <= TIGHT_K, (d["y_err"], d["cache_err"])


@pytest.mark.parametrize("row", [r for r in rm.ROWS if rm.is_split_row(r)], ids=[r["id"] for r in rm.ROWS if rm.is_split_row(r)])
def test_route_matrix_f16_control_misses_the_bar(row, records, error_report):
    d = records[(row["id"], True)]
    _report(error_report, d)
    assert d["trace_ok"], ("tile routes", d["expect"], d["got"], d["paths"])
    tiles = [t for ch in d["got"] for t in ch]
    assert all(t.endswith("split0") == (t.split()[0] in rm.ONE_PRODUCT) for t in tiles), tiles
    if any(t.endswith("split0") for t in tiles):
        assert d["err"] > TIGHT_K, (d["y_err"], d["cache_err"])
    else:
        assert d["err"] <= TIGHT_K, (d["y_err"], d["cache_err"])
