"""CPU: the plan of a wekws_hip_forward_streams call (wekws_amd/csrc/route.h: plan_streams), swept through the hooks library
(wekws_hip_debug_streams_plan) against a short restatement -- and the new entry points in the built library."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import forward_streams_matrix as fm
from tests import route_matrix as rm
from wekws_amd import _capi, pack
from wekws_amd.utils import synth

CUS = 256
SYMBOLS = ["wekws_hip_stream_cache_create", "wekws_hip_stream_cache_destroy", "wekws_hip_stream_cache_reset",
           "wekws_hip_stream_cache_read", "wekws_hip_stream_cache_write", "wekws_hip_forward_streams"]


def test_the_six_entry_points_are_exported():
    for path in (_capi.lib_path(), rm.hooks_path()):
        assert os.path.exists(path), f"{path} is missing: __graft_entry__.build()"
        lib = C.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(lib, name), (path, name)
    assert all(name in _capi.SIGNATURES for name in SYMBOLS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wekws_hip.h")).read()
    assert all(f" {name}(" in header for name in SYMBOLS)
    assert "#define WEKWS_HIP_ABI_VERSION 2 " in header            # additions only


@pytest.fixture(scope="module")
def lib():
    return fm.type_plan(C.CDLL(rm.hooks_path()))


def plan(lib, cfg, Tcap, frames, cus=CUS, opts=None):
    return fm.plan(lib, cfg, Tcap, frames, cus, opts)


def restated(frames, slots):
    """Live rows by frame count, largest first, ties in call order; a group: rows of equal count, at most `slots` (0: any number)."""
    order = sorted((b for b, n in enumerate(frames) if n > 0), key=lambda b: -frames[b])
    groups = []
    for b in order:
        if groups and groups[-1][0] == frames[b] and (not slots or len(groups[-1][1]) < slots):
            groups[-1][1].append(b)
        else:
            groups.append((frames[b], [b]))
    return order, groups


def frame_cases(rng, B, Tcap):
    distinct = [1 + (i % Tcap) for i in range(B)]
    mixed = [int(v) for v in rng.integers(-2, Tcap + 1, size=B)]
    one = [0] * B
    one[B // 2] = Tcap
    return {"all equal": [min(10, Tcap)] * B, "all distinct": [int(v) for v in rng.permutation(distinct)],
            "zeros and negatives mixed in": mixed, "one live row": one, "none live": [0, -1] * (B // 2) + [0] * (B % 2),
            "three counts": [int(v) for v in rng.permutation(np.resize([min(9, Tcap), min(10, Tcap), Tcap], B))]}


# (model, Tcap, B, expected kind): Tcap at and one beyond the table-driven kernels' tiles; B off the multiples of U at 2 / 4 x CUs
SWEEP = [("ds_tcn_h256", 16, 5, "ds256_stream"), ("ds_tcn_h256", 16, 1031, "ds256_stream"), ("ds_tcn_h256", 10, 7, "ds256_stream"),
         ("ds_tcn_h256", 17, 5, "grouped"), ("ds_tcn_h256_ctc", 16, 5, "grouped"),
         ("ds_tcn_h64", 16, 5, "grouped"), ("mdtc_h64", 16, 6, "grouped"), ("gru_2x128", 16, 6, "grouped"), ("gru_2x128", 40, 3, "grouped"),
         ("fsmn_ctc300", 16, 5, "fsmn_f16"), ("fsmn_ctc300", 16, 2 * CUS + 3, "fsmn_f16"), ("fsmn_ctc300", 16, 4 * CUS + 3, "fsmn_f16"),
         ("fsmn_ctc300", 32, 2 * CUS + 1, "fsmn_f16"), ("fsmn_ctc300", 64, 9, "fsmn_f16"), ("fsmn_ctc300", 65, 9, "grouped"),
         ("fsmn_small", 12, 6, "fsmn_f16"), ("fsmn_small", 16, 4 * CUS + 3, "fsmn_f16")]


@pytest.mark.parametrize("name,Tcap,B,kind", SWEEP)
def test_plan_sweep(lib, name, Tcap, B, kind):
    cfg = synth.MODEL_CONFIGS[name]
    rng = np.random.default_rng(B * 131 + Tcap)
    for what, frames in frame_cases(rng, B, Tcap).items():
        p = plan(lib, cfg, Tcap, frames)
        key = (name, Tcap, B, what)
        live = [b for b, n in enumerate(frames) if n > 0]
        assert p["live"] == len(live) and p["max_T"] == max([frames[b] for b in live] + [0]), key
        if not live:
            assert p["ngroups"] == 0 and p["order"] == [], key
            continue
        assert p["kind"] == kind, (key, p["why"])
        # every live row exactly once, skipped rows nowhere; rows sharing a group have equal T
        assert sorted(p["order"]) == live, key
        assert sorted(b for _, rows in p["groups"] for b in rows) == live, key
        assert all(frames[b] == T for T, rows in p["groups"] for b in rows), key
        if kind == "ds256_stream":
            slots = 1
            assert rm.FAMILIES[p["family"]] == "ds256_stream" and p["conv_grid"] == len(live), key
        elif kind == "fsmn_f16":
            r = rm.fsmn_route(lib, cfg, len(live), p["max_T"], cus=CUS)      # the instance of (live rows, largest T)
            slots = r["u"]
            assert (p["nt"], p["u"], p["head_slices"], p["fsmn_lds"]) == (r["nt"], r["u"], r["head_slices"], r["lds"]), key
            assert p["fsmn_grid"] == p["ngroups"], key
        else:
            slots = 0
            assert p["why"], key
        assert p["slots"] == slots, key
        assert all(len(rows) <= slots for _, rows in p["groups"]) or not slots, key
        order, groups = restated(frames, slots)
        assert p["order"] == order and p["groups"] == groups, key


def test_packing_really_packs(lib):
    """The sweep's large FSMN calls take u = 2 and u = 4, and B is no multiple of U: short groups exist."""
    for name, B, u in (("fsmn_ctc300", 2 * CUS + 3, 2), ("fsmn_small", 4 * CUS + 3, 4)):
        cfg = synth.MODEL_CONFIGS[name]
        frames = [int(v) for v in np.random.default_rng(1).permutation(np.resize([1, 7, 16], B))]
        p = plan(lib, cfg, 16, frames)
        assert p["u"] == u and p["slots"] == u
        sizes = [len(rows) for _, rows in p["groups"]]
        assert max(sizes) == u and min(sizes) < u and len(p["groups"]) == sum(-(-frames.count(T) // u) for T in (1, 7, 16))
    # the STREAM option off: no table-driven conv kernel
    assert plan(lib, synth.MODEL_CONFIGS["ds_tcn_h256"], 16, [10] * 5, opts={"stream": 0})["kind"] == "grouped"


# ---------------------------------------------------------------------------------------------------------------------------------
# The case table of the GPU tests (tests/forward_streams_matrix.py) reaches what it claims: a change of select_fsmn_route or
# plan_streams that quietly stops reaching an instance fails here, without a device.
def case_plans(lib, case):
    return [plan(lib, fm.case_config(case), case["Tcap"], frames) for frames in fm.plan_calls(case, CUS)]


@pytest.mark.parametrize("case", [c for c in fm.CASES if not c.get("device_only")], ids=lambda c: c["id"])
def test_matrix_case_has_the_plan_it_claims(lib, case):
    want = case["expect"]
    for p in case_plans(lib, case):
        assert p["kind"] == want["kind"], (case["id"], p["kind"], p["why"])
        if want["kind"] == "fsmn_f16":
            assert (p["nt"], p["u"]) == (want["nt"], want["u"]), (case["id"], p["nt"], p["u"], p["live"], p["max_T"])
        elif want["kind"] == "ds256_stream":
            assert rm.FAMILIES[p["family"]] == "ds256_stream" and p["split"] == want["split"], (case["id"], p["family"], p["split"])
        else:
            assert p["why"] == want["why"], (case["id"], p["why"])


def test_matrix_reaches_every_table_driven_instance(lib):
    """The FSMN cases together: exactly the seven (nt, u) of the switch in fsmn_f16_rows.hip -- parsed from it --; the DS-TCN
    cases: both splits of ds256_stream; group a alone already holds all seven, so the oracle sees each of them."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wekws_amd", "csrc", "fsmn_f16_rows.hip")).read()
    import re
    switch = sorted({(int(a), int(b)) for a, b in re.findall(r"case (\d)(\d):", src)})          # case nt * 10 + u
    assert switch == sorted(fm.FSMN_INSTANCES), switch
    got = {(p["nt"], p["u"]) for c in fm.FSMN_CASES for p in case_plans(lib, c)}
    assert sorted(got) == switch, sorted(got)
    assert {(p["nt"], p["u"]) for c in fm.NONFINITE_CASES for p in case_plans(lib, c)} == {(1, 2), (2, 2)}
    splits = {p["split"] for c in fm.DS256_CASES for p in case_plans(lib, c) if p["kind"] == "ds256_stream"}
    assert splits == {0, 1}, splits
    whys = {c["expect"]["why"] for c in fm.GROUPED_CASES}
    assert whys == {fm.PADDED, fm.WHY_DS_TILE, fm.WHY_FSMN_TILE, fm.WHY_NO_CONV, fm.WHY_GRU}


def test_matrix_frame_counts_are_what_the_cases_need(lib):
    """Group a: counts from the tile edges, a row at Tcap (but for the 64-frame-stride case), rows with 0 and -1 frames, ids a
    permutation; packed cases: a count whose rows are no multiple of u, a count held by ONE row (a group with one live slot), and a
    count whose uniform call over all B rows takes the same instance (what the bit-identity is asserted against)."""
    for case in fm.FSMN_CASES:
        ids, fr = fm.frames_of(case, CUS)
        nt, u = case["expect"]["nt"], case["expect"]["u"]
        live = [n for n in fr if n > 0]
        assert len(set(ids)) == len(ids) == len(fr) and max(ids) < len(fr) + 2 and ids != sorted(ids), case["id"]
        assert 0 in fr and -1 in fr and set(live) <= set(fm.EDGES) | {20}, case["id"]
        assert case["Tcap"] in fr or case["id"].endswith("stride64"), case["id"]
        p = plan(lib, fm.case_config(case), case["Tcap"], fr)
        sizes = [len(rows) for _, rows in p["groups"]]
        if u > 1:
            assert any(live.count(T) % u for T in set(live)) and 1 in [live.count(T) for T in set(live)], case["id"]
            assert min(sizes) == 1 and max(sizes) == u, case["id"]
        same = [T for T in set(live)
                if (lambda r: (r["nt"], r["u"]))(rm.fsmn_route(lib, fm.case_config(case), len(fr), T, cus=CUS)) == (nt, u)]
        assert same, case["id"]
    # the stride case: Tcap = 64, nothing above 20 frames
    ids, fr = fm.frames_of(fm.BY_ID["fsmn/nt2_stride64"], CUS)
    assert max(fr) == 20
    # group e: every row live, so a poisoned row has a slot-mate
    for case in fm.NONFINITE_CASES:
        ids, fr = fm.nonfinite_frames(case, CUS)
        assert min(fr) > 0 and sorted(ids) == list(range(len(fr)))
