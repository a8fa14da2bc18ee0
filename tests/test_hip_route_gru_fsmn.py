"""GPU: the GRU and FSMN routes on the device.  A child process with the TEST build of the library (libwekws_hip_hooks.so: its route
trace) -- tests/tools/route_gru_fsmn_cases.py, run once -- makes
  * the recipe calls (tests/route_matrix.py: GRU_CALLS, FSMN_CALLS): the trace of the forward must be the route route.h predicts on
    the CPU (wekws_hip_debug_gru_route / _fsmn_route), the launch that ran and not a neighbour: the GRU's family, tiles, slots,
    variant and where its non-finite pass ran; every FSMN tile's frame tiles, utterances per workgroup, head slices, grid and LDS;
  * every row of the GRU / FSMN route matrix (tests/route_matrix_rnn.py), and per row:
      - the trace of every chunk equals the literal prediction the CPU suite checks against route.h, and the path is the kernel
        family's (3 GRU, 4 FSMN, 2 the any-shape plan): the row ran the kernel it is named for;
      - every chunk's output, compared on its own, and the state (GRU: after EVERY chunk; FSMN: the final cache) meet the tight
        bar (tests/helpers.py::TIGHT_K) against the float64 oracle (four named CTC-head rows take each class's scale over the
        row's whole stream: tests/route_matrix_rnn.py::_fsmn_rows);
  * the negative control: the rows of control_rows() -- between them every route tuple -- rerun with the weight matrix that is
    least visible for the row on the CPU rounded to fp16, against the oracle of the UNROUNDED weights: the same trace, and the bar
    MISSED.  The comparison sees a lost lo(w) term through this kernel's outputs on the device.
The measured error per route tuple goes to the session's error report (tests/conftest.py::error_report)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from tests import route_matrix as rm
from tests import route_matrix_rnn as rr
from tests.helpers import TIGHT_K
from wekws_amd.utils import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "tools", "route_gru_fsmn_cases.py")


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """(traces of the recipe calls, records of the rows) of the one child process."""
    hooks = rm.hooks_path()
    assert os.path.exists(hooks), f"{hooks} is missing: make -C wekws_amd/csrc hooks (or __graft_entry__.build())"
    out = str(tmp_path_factory.mktemp("route_gru_fsmn") / "records.jsonl")
    env = dict(os.environ, WEKWS_HIP_LIB=hooks)
    r = subprocess.run([sys.executable, CASES, out], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    traces = {(d["model"], d["B"], d["T"]): d for d in map(json.loads, (l for l in r.stdout.splitlines() if l.startswith("{")))}
    recs = {}
    with open(out) as f:
        for line in f:
            d = json.loads(line)
            recs[(d["id"], d["control"])] = d
    return traces, recs


@pytest.fixture(scope="module")
def traces(child):
    return child[0]


@pytest.fixture(scope="module")
def records(child):
    return child[1]


@pytest.mark.parametrize("name,B,T", rm.GRU_CALLS + rm.FSMN_CALLS)
def test_traced_route_is_route_h(traces, name, B, T):
    lib = rm.type_hooks(C.CDLL(rm.hooks_path()))
    cfg = synth.MODEL_CONFIGS[name]
    d = traces[(name, B, T)]
    if cfg["backbone"]["type"] == "gru":
        r = rm.gru_route(lib, cfg, B, T, cus=d["cus"])
        want = [rm.GRU_FAMILIES.index(r["family"])] + rm.gru_record(r)[1:]
        assert d["path"] == 3 and d["records"] == [want], (d, want)
    else:
        want = []
        for i in range(d["ntiles"]):
            want.append(rm.fsmn_record(rm.fsmn_route(lib, cfg, B, T, tile=i, cus=d["cus"])))
        assert d["path"] == 4 and d["records"] == want, (d, want)


def _report(error_report, row, d, pick):
    """Per route tuple, the error of the CHUNKS that ran it (a GRU chunk is one route; the tiles of one FSMN call share the
    call's figure, an upper bound for each of them; the any-shape plan: the row's)."""
    plan, chunks = rr.EXPECT[row["id"]]
    for j, e in enumerate(d["chunk_err"]):
        if plan == "generic":
            tuples = {("any_shape",)}
        elif row["kind"] == "gru":
            tuples = {rr.gru_tuple(chunks[j])}
        else:
            tuples = {rr.fsmn_tuple(rec, i) for i, rec in enumerate(chunks[j])}
        for t in tuples:
            key = f"route_matrix/{row['kind']}/{'control/' if d['control'] else ''}{rr.tuple_key(row, t)}"
            error_report[key] = pick(error_report.get(key, e), e)


@pytest.mark.parametrize("row", rr.ROWS, ids=[r["id"] for r in rr.ROWS])
def test_gru_fsmn_row(row, records, error_report):
    d = records[(row["id"], False)]
    _report(error_report, row, d, max)
    assert d["trace_ok"], ("routes", d["expect"], d["got"], d["paths"])
    assert d["err"] <= TIGHT_K, (d["y_err"], d["state_err"])


@pytest.mark.parametrize("row", rr.control_rows(), ids=[r["id"] for r in rr.control_rows()])
def test_gru_fsmn_rounded_matrix_control_misses_the_bar(row, records, error_report):
    d = records[(row["id"], True)]
    _report(error_report, row, d, max)
    assert d["trace_ok"], ("routes", d["expect"], d["got"], d["paths"])
    assert d["err"] > TIGHT_K, (d["matrix"], d["y_err"], d["state_err"])
