"""GPU: the poisoned matrix (tests/nonfinite_matrix.py) and the named non-finite stress rows on the device.  A child process with
the TEST build of the library (libwekws_hip_hooks.so: its route trace) runs every derived row -- tests/tools/
nonfinite_matrix_cases.py --, and per row:
  * the trace of every call equals the base row's prediction: poison does not change the route, and the row ran the kernel it is
    there for;
  * finite / NaN / +Inf / -Inf classes equal the float64 oracle's at every position of every chunk's output and of the cache /
    state after every chunk;
  * the repaired part (a poisoned utterance in a call whose features or incoming cache / state are non-finite) meets TIGHT_K
    under every precision, f16 included: the repair is IEEE f32 whatever was asked;
  * everything else meets TIGHT_K too (under precision f16: the fast path's bar of tests/test_hip_nonfinite.py), and on the
    one-utterance-per-workgroup DS-TCN h256 routes the clean utterances equal the same call without poison bit for bit.
Then the stress rows, each in a child of its own under a time limit of its own (a hang in one ends that child, not the session):
the persistent kernels' list of noted utterances full and overflowing, and more poisoned workgroups than scratch slots.
Per-route maxima go to the session's error report under nonfinite_matrix/..."""
import json
import os
import subprocess
import sys

import pytest

from tests import nonfinite_matrix as nm
from tests import route_matrix as rm
from tests.helpers import TIGHT_K
from tests.tools.nonfinite_matrix_cases import STRESS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "tools", "nonfinite_matrix_cases.py")


ENDED_BADLY = []          # children that ended by a time limit or a signal: nothing more is started on the GPU after one


def _child(args, out, timeout):
    """One child under its own time limit.  After a child that hung, faulted or aborted (time limit, exit by signal, abort) no
    further child is started: the remaining tests of this module fail at once, and what the child left is read first."""
    assert not ENDED_BADLY, f"not started: an earlier child ended badly ({ENDED_BADLY[0]}); find its cause from its records first"
    hooks = rm.hooks_path()
    assert os.path.exists(hooks), f"{hooks} is missing: make -C wekws_amd/csrc hooks (or __graft_entry__.build())"
    env = dict(os.environ, WEKWS_HIP_LIB=hooks)
    try:
        r = subprocess.run([sys.executable, CASES] + args, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        ENDED_BADLY.append(f"{args[:2]}: no end within {timeout} s")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        ENDED_BADLY.append(f"{args[:2]}: exit status {r.returncode}")
    recs = []
    if os.path.exists(out):
        with open(out) as f:
            recs = [json.loads(line) for line in f]
    return r, recs


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("nonfinite_matrix") / "records.jsonl")
    r, recs = _child(["matrix", out], out, 900)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, len(recs), r.stdout[-2000:], r.stderr[-6000:])
    return {d["id"]: d for d in recs}


@pytest.mark.parametrize("row", nm.ROWS, ids=[r["id"] for r in nm.ROWS])
def test_nonfinite_matrix_row(row, records, error_report):
    d = records[row["id"]]
    worst = max(d["err_repaired"] + d["err_clean"] if row["precision"] != "f16" else d["err_repaired"])
    for key in d["keys"]:
        k = "nonfinite_matrix/" + ("f16/" if row["precision"] == "f16" else "") + key
        error_report[k] = max(error_report.get(k, 0.0), worst)
    if nm.nothing_to_see(row):        # the poisoned utterances keep nothing finite that a weight has touched: classes alone speak here
        error_report["nonfinite_matrix/classes_only/" + row["id"]] = worst
    assert d["trace_ok"], ("routes", d["expect"], d["got"], d["paths"])
    assert d["class_ok"], "finite / NaN / +Inf / -Inf classes differ from the float64 oracle's"
    assert max(d["err_repaired"]) <= TIGHT_K, ("repaired utterances", d["err_repaired"])
    assert max(d["err_clean"]) <= (1.0 if row["precision"] == "f16" else TIGHT_K), ("clean part", d["err_clean"])
    assert d["bitwise"] in (None, True), "clean utterances of a one-utterance-per-workgroup h256 route changed"
    assert (d["bitwise"] is not None) == bool(row["kind"] == "conv" and row["base"]["model"].startswith("ds_tcn_h256")
                                              and nm.base_expect(row["base"])[0] != "generic" and len(row["bad"]) < row["base"]["B"]
                                              and all(" upw1 " in t and t.startswith("ds256") for ch in d["expect"] for t in ch))


def test_error_report_lists_every_route(records, error_report):
    segs = {r["id"]: nm.segments(r["base"]) for r in nm.ROWS}
    keys = {nm.tuple_key(r["kind"], segs[r["id"]][s][3]) for r in nm.ROWS if r["precision"] != "f16" for s, _, _ in r["claims"]}
    have = {k[len("nonfinite_matrix/"):] for k in error_report if k.startswith("nonfinite_matrix/")}
    for d in records.values():                                     # (a run of this test alone has not filled the report yet)
        have |= set(d["keys"])
    assert keys <= have, sorted(keys - have)
    assert {nm.tuple_key(k, t) for k, _, t in nm.universe() if t[0] != "padded"} <= keys


@pytest.mark.parametrize("name", sorted(STRESS))
def test_nonfinite_stress_row(name, records, tmp_path, error_report):
    """The row in a child of its own, after the matrix (its fixture comes first); 120 s is far above what a poisoned utterance costs (about a millisecond each, behind one
    another in a persistent workgroup) and well below a hang."""
    out = str(tmp_path / "stress.jsonl")
    r, recs = _child(["stress", name, out], out, 120)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    assert len(recs) == STRESS[name][8]
    for d in recs:
        k = f"nonfinite_matrix/stress/{name}"
        error_report[k] = max(error_report.get(k, 0.0), max(d["err_repaired"] + d["err_clean"]))
        assert d["trace_ok"], ("routes", d["expect"], d["got"], d["paths"])
        assert d["class_ok"] and d["finite_ok"], (d["repeat"], d["class_ok"], d["finite_ok"])
        assert max(d["err_repaired"]) <= TIGHT_K and max(d["err_clean"]) <= TIGHT_K, (d["repeat"], d["err_repaired"], d["err_clean"])
        assert d["bitwise"] in (None, True), "clean utterances changed"
        assert (d["bitwise"] is not None) == name.startswith(("nflist", "slots_conv_upw1"))
