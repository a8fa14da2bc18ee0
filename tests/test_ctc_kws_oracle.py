"""CPU: the host restatement of the CTC prefix beam search and keyword detection (tests/ctc_kws_ref.py) equals what the
reference's own functions computed (tests/golden/ctc_kws_golden.npz), bit for bit, on every golden case."""
import math

import numpy as np
import pytest

from tests import ctc_kws_golden as G
from tests import ctc_kws_ref as R

Z, META = G.load()


@pytest.mark.parametrize("case", META["offline"], ids=lambda c: c["name"])
def test_offline_cases_equal_reference(case):
    probs = Z[f"off/{case['name']}"]
    kws = [tuple(k) for k in case["keywords"]]
    ts = None if case["tokenset"] is None else set(case["tokenset"])
    for b, exp in enumerate(case["expect"]):
        k, score, start, end, status, beam = R.keyword_search(probs[b, :case["lengths"][b]], kws, case["score_beam"],
                                                             case["path_beam"], ts)
        assert status == 0
        assert G.oracle_beam(beam) == G.beam_expect(exp["beam"])
        assert (k, score, start, end) == (exp["hit"], G.fx(exp["score"]), exp["start"], exp["end"])


@pytest.mark.parametrize("case", META["stream"], ids=lambda c: c["name"])
def test_stream_cases_equal_reference(case):
    c = case["config"]
    sp = R.Spotter(c["keywords"], c["threshold"], c["min_frames"], c["max_frames"], c["interval_frames"], c["score_beam"],
                   c["path_beam"], c["downsampling"])
    names = [f"kw{k}" for k in range(len(c["keywords"]))]
    i = 0
    for st in case["steps"]:
        if st["op"] != "chunk":
            getattr(sp, st["op"])()
            continue
        rec = sp.step(Z[f"str/{case['name']}/{i}"])
        i += 1
        got = R.as_result_dict(rec, names)
        exp = st["result"]
        assert set(got) == set(exp)
        for key in exp:
            e = G.fx(exp[key]) if isinstance(exp[key], str) and key != "keyword" else exp[key]
            assert got[key] == e, key
        assert sp.hit_score == G.fx(st["hit_score"])
        assert (sp.total_frames, sp.last_active_pos) == (st["total_frames"], st["last_active_pos"])
        assert G.oracle_cur_hyps(sp.beam) == G.cur_hyps_expect(st["beam"])


def test_golden_cases_cover_the_issue_items():
    """The recorded cases exercise what they are named for (a case that silently stopped doing so proves nothing)."""
    off = {c["name"]: c for c in META["offline"]}
    shared = G.beam_expect(off["shared_nodes"]["expect"][0]["beam"])
    aba = [h for h in shared if h[0] == (1, 2, 1)][0]
    assert aba[2][0][1:] == (2, np.float32(.9).item())            # the first `a` reports frame 2 / prob 0.9
    ab = [h for h in shared if h[0] == (1, 2)][0]
    assert [n[1] for n in ab[2]] == [2, 1]
    assert off["beam_empties"]["expect"][0]["beam"] == []
    assert off["sublist_end"]["expect"][0]["hit"] is None and off["sublist_start"]["expect"][0]["hit"] == 0
    tie = G.beam_expect(off["score_tie"]["expect"][0]["beam"])
    assert tie[1][1] == tie[2][1] and [h[0] for h in tie[1:3]] == [(2,), (1,)]
    st = {c["name"]: c for c in META["stream"]}
    activations = sum(s.get("result", {}).get("state", 0) for c in META["stream"] for s in c["steps"])
    assert activations >= 5
    assert any(s.get("result") == {} for s in st["tiny_chunks_ds3"]["steps"] if s["op"] == "chunk")
    carried = [G.fx(s["hit_score"]) for s in st["score_carried"]["steps"]]
    assert min(carried) < 1.0 and all(s["result"].get("state") == 0 for s in st["score_carried"]["steps"] if s["result"])
    assert st["beam_empties"]["steps"][-1]["beam"] == []


def test_oracle_first_beam_deviations():
    # exact ties inside the top-k: lower index first (torch's CPU order on ties is implementation-defined)
    assert R.first_beam(np.array([.1, .3, .3, .05, .3], np.float32), 3, None) == [1, 2, 4]
    # NaN ranks above every number, takes a place, and is dropped by the 0.05 filter
    assert R.first_beam(np.array([.1, np.nan, .6, .2, .07], np.float32), 3, None) == [2, 3]
    # the token set filters after the top-k of the whole row
    assert R.first_beam(np.array([.1, .3, .4, .06, .02], np.float32), 3, {0, 3}) == [0]
    assert R.is_sublist((9, 1, 2), (1, 2)) == -1 and R.is_sublist((1, 2, 9), (1, 2)) == 0
    assert math.isnan(float(np.float32("nan")))


def test_oracle_inf_fails_the_stream_only():
    sp = R.Spotter([(1, 2)], 0.5)
    x = np.full((3, 5), .01, np.float32)
    x[:, 0] = .96
    x[1, 3] = np.inf
    assert sp.step(x)["status"] == R.EINVAL and sp.total_frames == 0
    sp.reset()
    assert sp.status == 0 and sp.step(x[:1])["status"] == 0
