"""GPU: KWSModel.forward_streams / wekws_hip_forward_streams -- the model step for any subset of the streams of a cache pool, every
row with its own frame count.  A child process with the TEST build of the library (its route trace) runs the cases once
(tests/tools/forward_streams_cases.py) and prints what it measured; the tests judge the records.

Yardsticks: the float64 oracle (oracle/kws_oracle.py) fed one stream at a time with ITS carried cache, at TIGHT_K = 2^-15
(tests/helpers.py); bit-identity where the same kernel instance runs -- KWSModel.forward on a row alone, the uniform call of the
same (nt, u), the bucketed step that BatchedKeyWordSpotter.forward made before (index_select, forward, index_copy_)."""
import json
import os
import subprocess
import sys

import pytest

from tests import route_matrix as rm
from tests.helpers import TIGHT_K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "tools", "forward_streams_cases.py")
DS256_STREAM = rm.FAMILIES.index("ds256_stream")
LIVE = [4, 4, 5]          # live rows of the schedule's three calls


@pytest.fixture(scope="module")
def records():
    hooks = rm.hooks_path()
    assert os.path.exists(hooks), f"{hooks} is missing: make -C wekws_amd/csrc hooks (or __graft_entry__.build())"
    r = subprocess.run([sys.executable, CASES], env=dict(os.environ, WEKWS_HIP_LIB=hooks), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def pick(records, **want):
    got = [r for r in records if all(r.get(k) == v for k, v in want.items())]
    assert got, want
    return got


def check_rows(rec, alone, bucketed):
    """Every row of a schedule record: live rows within the bar and identical where asked, the call's other bytes untouched."""
    assert rec["left_out_kept"], (rec["model"], rec["call"])
    live = 0
    for row in rec["rows"]:
        key = (rec["model"], rec["call"], row["row"], row["stream"], row["frames"])
        if row["frames"] <= 0:
            assert row["y_untouched"] and row["cache_kept"], key
            continue
        live += 1
        print(f"forward_streams {key}: y {row['y_err']:.3e} cache {row['cache_err']:.3e} of {TIGHT_K:.3e}")
        assert row["y_err"] <= TIGHT_K and row["cache_err"] <= TIGHT_K, (key, row["y_err"], row["cache_err"])
        assert row["tail_untouched"], key
        if alone:
            assert row["y_alone"] and row["cache_alone"], key
        if bucketed:
            assert row["y_bucketed"] and row["cache_bucketed"], key
    assert live == LIVE[rec["call"]]


def test_ds256_stream_schedule(records):
    """DS-TCN 4 x 256, kernel 8, 40-d input, a keyword head: one table-driven launch of ds256_stream per call."""
    recs = pick(records, kind="schedule", model="ds_tcn_h256")
    assert [r["call"] for r in recs] == [0, 1, 2]
    for rec in recs:
        assert rec["path"] == 1 and rec["ntiles"] == 1, rec["records"]
        family, nt, _, _, _, grid = rec["records"][0][:6]
        assert family == DS256_STREAM and nt == 1 and grid == LIVE[rec["call"]], rec["records"]
        check_rows(rec, alone=True, bucketed=True)


def test_fsmn_schedule(records):
    """The small CTC FSMN with the softmax on: one table-driven launch, one row per workgroup at this size."""
    recs = pick(records, kind="schedule", model="fsmn_ctc300")
    assert [r["call"] for r in recs] == [0, 1, 2]
    for rec in recs:
        assert rec["path"] == 4 and rec["ntiles"] == 1, rec["records"]
        _, nt, u, _, grid, _, ntiles = rec["records"][0][:7]
        assert (nt, u, grid, ntiles) == (1, 1, LIVE[rec["call"]], 1), rec["records"]
        # (a row alone and a bucket of the bucketed step trace (nt, u) = (1, 1) too at <= 16 frames: the same instance)
        check_rows(rec, alone=True, bucketed=True)


def test_fsmn_two_rows_per_workgroup(records):
    """2 x CUs + 3 rows, frames from {1, 7, 16}: (nt, u) = (1, 2), rows of equal frame count paired, partial groups."""
    rec = pick(records, kind="packed")[0]
    B = rec["B"]
    counts = {T: len([i for i in range(B) if [1, 7, 16][i % 3] == T]) for T in (1, 7, 16)}
    assert rec["path"] == 4 and rec["ntiles"] == 1
    _, nt, u, _, grid, _, _ = rec["records"][0][:7]
    assert (nt, u) == (1, 2) and grid == sum((n + 1) // 2 for n in counts.values()), (rec["records"], counts)
    assert any(n % 2 for n in counts.values())                    # some group is partial
    print(f"forward_streams packed: y {rec['y_err']:.3e} cache {rec['cache_err']:.3e} of {TIGHT_K:.3e}")
    assert rec["y_err"] <= TIGHT_K and rec["cache_err"] <= TIGHT_K, (rec["y_err"], rec["cache_err"])
    assert rec["tails"]
    for T, uni in rec["uniform"].items():
        assert uni["rows"] == counts[int(T)]
        # bit-identity only against a uniform call that traces the same instance
        assert uni["records"][0][1:3] == [1, 2], uni["records"]
        assert uni["identical"], T


@pytest.mark.parametrize("name,path", [("mdtc_h64", 1), ("gru_2x128", 3)])
def test_grouped_schedule(records, name, path):
    """No table-driven kernel: buckets inside the library, bit-identical to the bucketed step in Python (and so to a row alone
    only where a bucket holds one row: not asserted)."""
    recs = pick(records, kind="schedule", model=name)
    assert [r["call"] for r in recs] == [0, 1, 2]
    for rec in recs:
        buckets = len({row["frames"] for row in rec["rows"] if row["frames"] > 0})
        assert rec["path"] == path and rec["ntiles"] == buckets, (rec["path"], rec["ntiles"], buckets)
        check_rows(rec, alone=False, bucketed=True)


@pytest.mark.parametrize("name", ["ds_tcn_h256", "fsmn_ctc300"])
def test_nonfinite_rows_follow_the_table(records, name):
    """A NaN feature in one row, a +Inf in another stream's carried cache: those rows as the float64 oracle has them -- class by
    class, the finite values within the bar --, every other row of the call bit-identical to the call without the poison.
    That holds because these calls have five rows, so one row per workgroup (u = 1).  With u > 1 a poisoned slot sends every
    row of its WORKGROUP through the non-finite path: a slot-mate then has the oracle's values within the bar, not the clean call's
    bits, and only the rows of other workgroups are bit-identical (tests/test_hip_forward_streams_matrix.py, group e)."""
    rec = pick(records, kind="nonfinite", model=name)[0]
    assert sorted(r["row"] for r in rec["rows"] if r["poisoned"]) == [1, 3]
    for row in rec["rows"]:
        if row["poisoned"]:
            print(f"forward_streams nonfinite {name} row {row['row']}: y {row['y_err']:.3e} cache {row['cache_err']:.3e}")
            assert row["nonfinite"] > 0, row                      # the poison reached the reference's result
            assert row["y_err"] <= TIGHT_K and row["cache_err"] <= TIGHT_K, row
        else:
            assert row["identical"], row


def test_refusals_launch_nothing(records):
    rec = pick(records, kind="refusals")[0]
    assert sorted(rec["calls"]) == ["frames = Tcap + 1", "id = max_streams", "pool of another model", "repeated id"]
    for what, c in rec["calls"].items():
        assert c["rc"] == -1 and c["names_row"], (what, c)          # WEKWS_HIP_EINVAL
    assert "another model" in rec["calls"]["pool of another model"]["message"]
    assert rec["y_untouched"] and rec["good_call_same"]


def test_pipeline_equals_the_bucketed_step(records):
    """BatchedKeyWordSpotter over an FSMN, uneven chunks across streams: detections and posteriors bit for bit those of the
    bucketed step written out from the same front end and decoder."""
    rec = pick(records, kind="pipeline")[0]
    assert rec["calls"] == 7 and rec["rows"] > 10
    assert max(len(c) for c in rec["frame_counts"]) >= 2            # some call held rows of different frame counts
    assert all(p == 4 for p in rec["paths"]), rec["paths"]          # the FSMN kernel, table-driven
    assert rec["same_probs"] and rec["same_results"]
