"""GPU: every table-driven kernel instance and every grouped-path reason of wekws_hip_forward_streams, on the case table of
tests/forward_streams_matrix.py (tests/test_forward_streams_plan.py checks on the CPU that the table reaches what it claims).  A
child process with the TEST build of the library runs the cases once (tests/tools/forward_streams_matrix_cases.py) and prints what
it measured; the tests judge the records.

Yardsticks, none of them new: the float64 oracle fed each stream's carried cache at TIGHT_K = 2^-15, every live row compared
(the channel scales of the packed FSMN calls over the rows of one frame count: the reason stands in the child's fsmn_case);
F16_TOL for the one-fp16-product variant; bit-identity where the trace proves the same kernel instance (the uniform call of the
same (nt, u), a row alone, the bucketed step) and between a pool and its twin that synchronises after every call."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import pytest

from tests import forward_streams_matrix as fm
from tests import route_matrix as rm
from tests.helpers import F16_TOL, TIGHT_K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "tools", "forward_streams_matrix_cases.py")
DS256_STREAM = rm.FAMILIES.index("ds256_stream")
TRACE_CONV, TRACE_ANY_SHAPE, TRACE_GRU, TRACE_FSMN = 1, 2, 3, 4


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


def report(error_report, key, **figures):
    bar = figures.pop("bar", TIGHT_K)
    print(f"forward_streams/{key}: " + " ".join(f"{k} {v:.3e}" for k, v in figures.items()) + f" of {bar:.3e}")
    error_report[f"forward_streams/{key}"] = max(figures.values())


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fm.FSMN_CASES, ids=lambda c: c["id"])
def test_fsmn_instance(records, error_report, case):
    """a. One table-driven launch of the instance the case names, over rows whose frame counts sit on the tile edges: y[:T] and
    the cache of every live row against the oracle, everything else untouched, bit-identity to the uniform call of the same
    (nt, u) for at least one frame count."""
    rec = pick(records, kind="fsmn", id=case["id"])[0]
    ids, frames = fm.frames_of(case, rec["cus"])
    nt, u = case["expect"]["nt"], case["expect"]["u"]
    counts = {T: frames.count(T) for T in set(frames) if T > 0}
    assert rec["cus"] == fm.CUS and rec["B"] == fm.rows_of(case) and rec["c0_nonzero"]
    assert rec["path"] == TRACE_FSMN and rec["ntiles"] == 1, rec["records"]
    _, got_nt, got_u, slices, grid, _, ntiles = rec["records"][0][:7]
    assert (got_nt, got_u, ntiles) == (nt, u, 1), rec["records"]
    assert grid == sum(-(-n // u) for n in counts.values()), (grid, counts)
    if case["model"] == "fsmn_ctc300":
        assert slices == 8, rec["records"]                           # 3 workgroups on 256 CUs: the head over 8 slices each
    report(error_report, case["id"], y=rec["y_err"], cache=rec["cache_err"])
    assert sorted(int(T) for T in rec["counts"]) == sorted(counts)
    identical = 0
    for T, c in sorted(rec["counts"].items(), key=lambda kv: int(kv[0])):
        assert c["rows"] == counts[int(T)]
        print(f"  T = {T}: {c['rows']} rows, y {c['y_err']:.3e} cache {c['cache_err']:.3e}; worst row on its own scales: "
              f"y {c['y_own_scale']:.3e} (row {c['y_row']}) cache {c['cache_own_scale']:.3e} (row {c['cache_row']})")
        assert c["y_err"] <= TIGHT_K and c["cache_err"] <= TIGHT_K, (case["id"], T, c)
        if c["uniform"][1:3] == [nt, u]:                             # bit-identity only against the same instance
            assert c["identical"], (case["id"], T, c)
            identical += 1
    assert identical >= 1, (case["id"], rec["counts"])                # "the arithmetic is untouched" is checked for this instance
    assert rec["tails"] and rec["skipped"] == 2 and rec["skipped_untouched"] and rec["left_out_kept"], case["id"]


def test_fsmn_cases_ran_all_seven_instances(records):
    ran = {tuple(r["records"][0][1:3]) for r in records if r["kind"] == "fsmn"}
    assert sorted(ran) == sorted(fm.FSMN_INSTANCES), sorted(ran)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fm.DS256_CASES, ids=lambda c: c["id"])
def test_ds256_stream_variant(records, error_report, case):
    """b. ds256_stream's table-driven kernel with one fp16 product (split 0) and with the two-class softmax behind it: every row
    bit-identical to the same precision's forward / forward_softmax on the row alone, and within that precision's bar of the
    float64 oracle -- F16_TOL in units of max(1, max |ref|) for f16 (against the fp16-operand emulation as well), TIGHT_K otherwise."""
    rec = pick(records, kind="ds256", id=case["id"])[0]
    f16 = case["precision"] == "f16"
    _, frames = fm.frames_of(case)
    assert rec["path"] == TRACE_CONV and rec["ntiles"] == 1, rec["records"]
    family, nt, split, _, _, grid = rec["records"][0][:6]
    assert (family, nt, split, grid) == (DS256_STREAM, 1, case["expect"]["split"], sum(n > 0 for n in frames)), rec["records"]
    assert rec["effective"] == ("f16" if f16 else "f16x3")
    bar = F16_TOL if f16 else TIGHT_K
    assert [r["frames"] for r in rec["rows"]] == frames and rec["left_out_kept"]
    for row in rec["rows"]:
        if row["frames"] <= 0:
            assert row["y_untouched"] and row["cache_kept"], row
            continue
        figures = {k: row[k] for k in ("y_err", "cache_err", "y_emu", "cache_emu") if k in row}
        report(error_report, f"{case['id']}/row{row['row']}_T{row['frames']}", bar=bar, **figures)
        assert max(figures.values()) <= bar, row
        assert row["y_alone"] and row["cache_alone"] and row["tail_untouched"], row


# ---------------------------------------------------------------------------------------------------------------------------------
def buckets_traced(rec):
    """Uniform forwards of a grouped call, from its trace: a conv or GRU forward leaves one record per tile of 112 frames (one here),
    an FSMN forward one per tile of its call, each carrying the call's tile count."""
    if rec["path"] == TRACE_FSMN:
        n = sum(Fraction(1, r[6]) for r in rec["records"])
        assert n.denominator == 1, rec["records"]
        return int(n)
    return rec["ntiles"]


@pytest.mark.parametrize("case", fm.GROUPED_CASES, ids=lambda c: c["id"])
def test_grouped_case(records, error_report, case):
    """c. The grouped path (gather, the uniform forward, scatter) on rows longer than a tile, zero-padded models, the any-shape
    path, pooled heads, a cache of 195 floats and a CTC head with its softmax: every live row against the oracle and bit-identical
    to the bucketed step; one bucket per distinct frame count."""
    recs = pick(records, kind="grouped", id=case["id"])
    assert [r["call"] for r in recs] == [0, 1, 2]
    cfg = fm.case_config(case)
    generic = case["id"].startswith("grouped/generic")
    worst_y = worst_c = 0.0
    for rec in recs:
        frames = case["frames"][rec["call"]]
        buckets = len({n for n in frames if n > 0})
        if generic:                                                   # the any-shape path leaves no tile records
            assert rec["path"] == TRACE_ANY_SHAPE and rec["ntiles"] == 0, (rec["path"], rec["ntiles"])
        else:
            want = {"gru": TRACE_GRU, "fsmn": TRACE_FSMN}.get(cfg["backbone"]["type"], TRACE_CONV)
            assert rec["path"] == want and buckets_traced(rec) == buckets, (rec["path"], rec["ntiles"], buckets, rec["records"])
            if cfg["backbone"]["type"] == "fsmn" and case["Tcap"] > 64:
                assert max(r[6] for r in rec["records"]) == 2         # tiles chained through the workspace inside a bucket
        assert rec["left_out_kept"] and rec["warm_nonzero"], (case["id"], rec["call"])
        assert [r["frames"] for r in rec["rows"]] == frames
        if case["pooled"]:
            assert rec["y_shape"] == [5, cfg["output_dim"]], rec["y_shape"]
        else:
            assert rec["y_shape"] == [5, case["Tcap"], cfg["output_dim"]], rec["y_shape"]
        if case["cache_shape"]:
            assert rec["read_shape"] == list(case["cache_shape"]), rec["read_shape"]     # the caller's geometry, not the widened one
        for row in rec["rows"]:
            key = (case["id"], rec["call"], row["row"], row["stream"], row["frames"])
            if row["frames"] <= 0:
                assert row["y_untouched"] and row["cache_kept"], key
                continue
            worst_y, worst_c = max(worst_y, row["y_err"]), max(worst_c, row["cache_err"])
            assert row["y_err"] <= TIGHT_K and row["cache_err"] <= TIGHT_K, (key, row["y_err"], row["cache_err"])
            assert row["tail_untouched"] and row["y_bucketed"] and row["cache_bucketed"], (key, row)
    report(error_report, case["id"], y=worst_y, cache=worst_c)
    if case["pooled"]:
        ref = pick(records, kind="pooled_softmax", id=case["id"])[0]
        assert ref["refused"].startswith("IndexError") and ref["untouched"], ref


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,path", [("ds_tcn_h256", "table-driven"), ("mdtc_h64", "grouped")])
def test_pool_mechanics(records, name, path):
    """d. What the pool's comments state: the ring of four pinned row tables with nine calls in flight, the grouped scratch growing
    between calls nobody waited for, read / write at either parity, reset(None) at mixed parity, a call holding every stream, and
    three more refusals -- each on a pool and on a twin that synchronises after every call, bit for bit."""
    rec = pick(records, kind="pool", model=name)[0]
    assert rec["ring"] == dict(calls=9, same=True, distinct_ids=9, distinct_frames=9), rec["ring"]
    assert rec["grow"]["same"] and rec["grow"]["bucketed"], rec["grow"]
    if path == "grouped":                                             # three buckets, six, two: the second call outgrows the first
        assert [p[1] for p in rec["grow"]["paths"]] == [2, 4, 2], rec["grow"]
    assert rec["write_read"] == [True] * 3 and rec["write_step"] == [True] * 3, (rec["write_read"], rec["write_step"])
    ra = rec["reset_all"]
    assert ra["stepped"] == [True] * 5 + [False] * 2 and ra["zero"] and ra["next_call_same"] and ra["bucketed"] and ra["rows"] == fm.STREAMS, ra
    rf = rec["refusals"]
    for what in ("B > max_streams", "Tcap = 0"):
        assert rf[what]["rc"] == -1 and "forward_streams" in rf[what]["message"], (what, rf[what])       # WEKWS_HIP_EINVAL
    assert rf["set_precision"]["raised"].startswith("RuntimeError") and rf["set_precision"]["handle_changed"], rf["set_precision"]
    assert rf["y_untouched"] and rf["streams_untouched"], rf


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fm.NONFINITE_CASES, ids=lambda c: c["id"])
def test_nonfinite_in_packed_groups(records, error_report, case):
    """e. With two rows per workgroup a NaN feature or a +Inf in a carried cache sends the WHOLE workgroup through the non-finite
    path: the poisoned rows and their slot-mates have the oracle's classes and, on the finite values, its values within the bar
    (a slot-mate is NOT bit-identical to the clean call: other arithmetic); every row of another workgroup is."""
    rec = pick(records, kind="nonfinite_packed", id=case["id"])[0]
    nt, u = case["expect"]["nt"], case["expect"]["u"]
    assert rec["path"] == TRACE_FSMN and rec["records"][0][1:3] == [nt, u], rec["records"]
    assert all(len(g) == u for g in rec["groups"]) and rec["groups"][0] != rec["groups"][1], rec["groups"]
    assert rec["nan_row"] in rec["groups"][0] and rec["inf_row"] in rec["groups"][1]
    assert len(rec["touched"]) == 2 * u and sum(r["poisoned"] for r in rec["touched"]) == 2
    for row in rec["touched"]:
        report(error_report, f"{case['id']}/row{row['row']}_{'poisoned' if row['poisoned'] else 'slot_mate'}", y=row["y_err"], cache=row["cache_err"])
        assert row["y_err"] <= TIGHT_K and row["cache_err"] <= TIGHT_K and row["tail_untouched"], row
        if row["poisoned"]:
            assert row["nonfinite"] > 0 and not row["same_as_clean"], row      # the poison reached the reference's result
        else:
            assert row["nonfinite"] == 0, row
    assert rec["others"] == rec["B"] - 2 * u and rec["others_identical"], (rec["others"], rec["others_identical"])


def test_added_child_time(records):
    """The child's time per section, for the record (printed, not judged: a run-time budget is no property of the kernels)."""
    for r in pick(records, kind="seconds"):
        print(f"forward_streams matrix child: {r['section']} {r['seconds']} s")
