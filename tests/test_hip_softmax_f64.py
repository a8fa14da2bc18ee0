"""GPU: softmax_rows_kernel (forward_softmax) and softmax_topk_kernel (wekws_hip_softmax_topk) against the FLOAT64 oracle
(oracle/topk_oracle.py::softmax_f64 / softmax_topk_f64) in softmax_units at K_SOFTMAX (tests/helpers.py), over the matrix of
tests/softmax_matrix.py: every class count around the kernels' vector width and lane stride, masked (-Inf) and poisoned (NaN,
+Inf) rows.  A child process with the TEST build of the library (libwekws_hip_hooks.so: wekws_hip_debug_softmax_rows reaches the
in-place kernel with chosen logits) runs every row once -- tests/tools/softmax_matrix_cases.py, one timeout -- and records; per row:
  * classes first: got and the oracle are finite / the exact zero of a masked class / NaN at the same positions (a mismatch is an
    infinite figure), then every posterior within K_SOFTMAX units -- a RELATIVE bar: an all-zero tail or 8 % off in every class of
    a 2599-class row passed the absolute bars (1e-6, 1e-4, 2^-15) that were the only checks before;
  * the sentinel rows around the in-place buffer, around the top-k outputs and the logits themselves come back bit-identical;
  * top-k indices exactly the oracle's (a stable order on the logits: masked classes after the finite ones by ascending index, NaN
    never selected, (-1, 0) where nothing is left), the probabilities in the same unit.
The five ties: forward(softmax = 1) equals the hook applied to the same call's logits bit for bit, one model per forward path and
one whose activation is the softmax -- what the hook measures is what the product runs.
The worst figure per (kernel, law) goes to the session's error report under softmax_f64/..."""
import json
import os
import subprocess
import sys

import pytest

from tests import softmax_matrix as sm
from tests.fbank_matrix import hooks_path
from tests.helpers import K_SOFTMAX

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "tools", "softmax_matrix_cases.py")
TIES = ("conv_ctc", "gru", "fsmn", "any_shape", "exported_softmax")


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    hooks = hooks_path()
    assert os.path.exists(hooks), f"{hooks} is missing: make -C wekws_amd/csrc hooks (or __graft_entry__.build())"
    out = str(tmp_path_factory.mktemp("softmax_matrix") / "records.jsonl")
    env = dict(os.environ, WEKWS_HIP_LIB=hooks)
    r = subprocess.run([sys.executable, CASES, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    with open(out) as f:
        return {d["id"]: d for d in map(json.loads, f)}


@pytest.mark.parametrize("row", sm.ROWS, ids=sm.IDS)
def test_softmax_matrix_row(row, records, error_report):
    d = records[row.id]
    print(row.id, "k", row.k, "rows u", d["rows_u"], d["rows_worst"], "topk u", d["topk_u"], d["topk_worst"])
    for kernel in ("rows", "topk"):
        key = f"softmax_f64/{kernel}/{row.law}"
        error_report[key] = max(error_report.get(key, 0.0), d[kernel + "_u"])
    assert (d["K"], d["rows"], d["k"]) == (row.K, row.rows, row.k)
    assert d["rows_sentinels"], "softmax_rows_kernel wrote outside its rows"
    assert d["rows_u"] <= K_SOFTMAX, (d["rows_u"], d["rows_worst"])
    assert d["rows_nan"] == (row.rows * row.K if row.law in sm.NAN_ROW_LAWS else 0)
    assert d["topk_sentinels"], "softmax_topk_kernel wrote outside its outputs, or to its logits"
    assert d["topk_idx_in_range"]
    assert d["topk_idx_equal"], d.get("topk_first_mismatch")
    assert d["topk_u"] <= K_SOFTMAX, (d["topk_u"], d["topk_worst"])


@pytest.mark.parametrize("name", TIES)
def test_forward_softmax_is_the_hook_on_the_logits(name, records, error_report):
    d = records["tie/" + name]
    print(d)
    error_report[f"softmax_f64/tie/{name}"] = d["u"]
    assert d["path"] == d["want_path"] and d["same_path"], "the model did not take the forward path it is here for"
    assert d["rows"] == 15 and d["shape_ok"] and d["changed"]
    assert d["equal"], "forward(softmax = 1) is not the hook applied to forward(softmax = 0)"
    assert d["equal_softmax0"] is (True if name == "exported_softmax" else None)
    assert d["u"] <= K_SOFTMAX
