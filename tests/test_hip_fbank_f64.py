"""GPU: the fbank kernel against the FLOAT64 evaluation of the pipeline (oracle/fbank_oracle.py::fbank_f64) at the tight bar
K_FBANK (tests/helpers.py), over the variant matrix of tests/fbank_matrix.py.  A child process with the TEST build of the library
(libwekws_hip_hooks.so: the launch record, the table hook) runs every row once -- tests/tools/fbank_matrix_cases.py, one timeout --
and per row:
  * the launch ran the variant the row is named for (rounds, paired or per-sample loads, sample type from the launch record);
  * every bin of every frame of every utterance (noise, sine, the int16 ramp, silence) has fbank_units <= K_FBANK.  The large-batch
    rows check a fixed sample of utterances (first, last, either side of every wave-stride wrap, one in 97) and every utterance,
    bit for bit, against the same utterances run in batches of 8;
  * float and int16 samples give the same features bit for bit;
  * the mel weights in the handle's device table are the float64 oracle's bank (fbank_oracle.mel_bank), bit for bit.
Negative controls, on the rows named for them (a perturbed device table, the handle restored afterwards):
  * one mel weight x (1 + 2^-12) misses the bar in its bin and nowhere else;
  * the mel bank computed in double and twiddles on a 2^-18 grid miss it;
  * both twiddle tables rebuilt by the reference's float32 recurrence stay INSIDE it: that table is 1.5 ulp of 1 off at worst and
    the reference's own pipeline is inside the bar (K_FBANK's calibration notes) -- the old bars were not wide because of the
    reference's FFT but because the arbiter's mel bank was built with another logarithm than the reference's.
The worst figure per variant goes to the session's error report under fbank_f64/..."""
import json
import os
import subprocess
import sys

import pytest

from tests import fbank_matrix as fm
from tests.helpers import CONTROL_MARGIN, K_FBANK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "tools", "fbank_matrix_cases.py")


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    hooks = fm.hooks_path()
    assert os.path.exists(hooks), f"{hooks} is missing: make -C wekws_amd/csrc hooks (or __graft_entry__.build())"
    out = str(tmp_path_factory.mktemp("fbank_matrix") / "records.jsonl")
    env = dict(os.environ, WEKWS_HIP_LIB=hooks)
    r = subprocess.run([sys.executable, CASES, out], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    with open(out) as f:
        return {d["id"]: d for d in map(json.loads, f)}


@pytest.mark.parametrize("row", fm.ROWS, ids=[r["id"] for r in fm.ROWS])
def test_fbank_matrix_row(row, records, error_report):
    d = records[row["id"]]
    print(row["id"], d["variant"], "B", d["B"], "grid", d["grid"], "of", d["resident"], "u", d["u"], d["u_kind"], "worst", d["worst"])
    key = "fbank_f64/" + d["variant"].replace(" ", "_") + ("/" + "_".join(map(str, row["grid"])) if row["grid"] else "")
    error_report[key] = max(error_report.get(key, 0.0), d["u"])
    assert d["variant"] == row["variant"], (d["variant"], row["variant"])
    assert d["launch"] == [d["B"], row["nsamp"], row["nframes"]]
    if row["grid"] is None:
        assert d["grid"] == d["wanted_groups"] <= d["resident"] and d["checked"] == d["B"] == row["B"]
    elif row["grid"][0] == "over":                     # persistent waves: the grid is one resident round, every wave walks 2+ strides
        assert d["grid"] == d["resident"] and d["wanted_groups"] > 2 * d["resident"]
        assert d["batches_of_8_equal"]
    else:                                              # just under: one workgroup per tile, the last resident slots unused
        assert d["resident"] - 6 <= d["grid"] == d["wanted_groups"] < d["resident"]
        assert d["batches_of_8_equal"]
    assert d["other_type_equal"], "float and int16 samples differ"
    assert d["bank_equal"], "the device table's mel weights are not the oracle's bank"
    assert d["u"] <= K_FBANK, (d["u"], d["u_kind"], d["worst"])


@pytest.mark.parametrize("rid", fm.CONTROL_ROWS)
def test_negative_controls(rid, records, error_report):
    d = records[rid]
    c = d["controls"]
    print(rid, c)
    for name, v in c.items():
        error_report[f"fbank_f64/control/{name}/{rid}"] = v["u"]
    assert set(c) == set(fm.CONTROLS) and d["restored"]
    assert c["weight"]["u_bin"] > CONTROL_MARGIN * K_FBANK and c["weight"]["u_other"] <= K_FBANK, c["weight"]
    assert c["mel_double"]["u"] > K_FBANK and c["coarse_twiddle"]["u"] > K_FBANK, c
    assert c["twiddle"]["u"] <= K_FBANK, c["twiddle"]
