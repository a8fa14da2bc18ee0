"""GPU: every stream of the batched CTC spotter with its own keyword set (wekws_hip_ctc_kws_add_set / _drop_set / _assign /
_search_sets; wekws_amd.ctc, wekws_amd.stream).  The oracle of a stream is the host restatement of ONE KeyWordSpotter built
with the keywords, the token set and the threshold of the stream's set (tests/ctc_kws_ref.py::Spotter), replaced by a fresh
one whenever the stream is assigned; records, beams and hit scores are compared bit for bit."""
import numpy as np
import pytest
import torch

from tests import ctc_kws_golden as G
from tests import ctc_kws_ref as R
from tests.test_hip_ctc_kws import check_record, dev, peaky
from wekws_amd import _capi, ctc

pytestmark = pytest.mark.gpu

CFG = dict(min_frames=0, max_frames=80, interval_frames=10, score_beam=3, path_beam=20, downsampling=1)


def kwset(keywords, threshold, tokenset=None):
    return dict(keywords=[tuple(k) for k in keywords], threshold=threshold, tokenset=tokenset)


def oracle(s, c=CFG, cap=None):
    o = R.Spotter(s["keywords"], s["threshold"], c["min_frames"], c["max_frames"], c["interval_frames"], c["score_beam"],
                  c["path_beam"], c["downsampling"], capacity=cap)
    if s["tokenset"] is not None:
        o.tokenset = set(s["tokenset"])
    return o


def spotter(n, V, sets, c=CFG, cap=None):
    """A device spotter whose set 0 is sets[0] (default token set) and whose registered sets are the others; their ids."""
    dv = ctc.StreamingKeywordSpotter(n, sets[0]["keywords"], sets[0]["threshold"], c["min_frames"], c["max_frames"],
                                     c["interval_frames"], c["score_beam"], c["path_beam"], c["downsampling"], vocab=V,
                                     prefix_capacity=cap)
    return dv, [0] + [dv.add_keywords(s["keywords"], s["threshold"], s["tokenset"]) for s in sets[1:]]


def rows(V, toks, p=.9):
    """One frame per token: that token at p, the others far below the 0.05 filter."""
    x = np.full((len(toks), V), (1 - p) / (V - 1), np.float32)
    x[np.arange(len(toks)), toks] = p
    return x


def step_all(dv, x, streams):
    return dv.step_records(dev(np.stack(x)), None, streams)


# ----------------------------------------------------------------------------------------------- fuzz vs the oracle
@pytest.mark.parametrize("cap", [None, 12])
@pytest.mark.parametrize("seed", range(4))
def test_fuzz_streams_with_their_own_sets_against_oracle(seed, cap):
    """3 to 5 sets (one without keywords, one with an explicit token set, thresholds differ), streams assigned at random,
    random chunkings, subsets, orders, resets and re-assignments; both kernel instances (beams up to 4 / 32, and beyond)."""
    rng = np.random.default_rng(300 + seed)
    V = [20, 33, 300, 2599][seed]
    c = dict(min_frames=int(rng.integers(0, 8)), max_frames=int(rng.integers(20, 120)), interval_frames=int(rng.integers(5, 60)),
             score_beam=[3, 8, 6, 2][seed], path_beam=[20, 64, 1, 20][seed], downsampling=int(rng.choice([1, 3])))
    top = min(V, 30)

    def some_keywords(k):
        return [tuple(int(x) for x in rng.choice(np.arange(1, top), int(rng.integers(1, 4)), replace=False)) for _ in range(k)]

    nsets = int(rng.integers(3, 6))
    counts = [int(rng.integers(1, 4)) for _ in range(nsets)]
    counts[int(rng.integers(1, nsets))] = 0                      # a registered set without keywords
    sets = [kwset(some_keywords(k), float(rng.uniform(0, .7))) for k in counts]
    e = int(rng.choice([i for i in range(1, nsets) if counts[i]]))
    sets[e]["tokenset"] = sorted({int(t) for t in rng.choice(top, 6)} | {t for k in sets[e]["keywords"][:1] for t in k} | {V - 1})
    pool = [k for s in sets for k in s["keywords"]]
    n = 12
    dv, ids = spotter(n, V, sets, c, cap)
    assert ids == list(range(nsets))
    own = rng.integers(0, nsets, n)
    own[0] = 0                                                   # (stream 0 is never assigned at all)
    for i in range(1, nsets):
        dv.assign([s for s in range(1, n) if own[s] == i], i)
    orc = [oracle(sets[own[s]], c, cap) for s in range(n)]
    for _ in range(10 if cap is None else 30):
        sub = rng.permutation(n)[:int(rng.integers(1, n + 1))]
        T = int(rng.integers(0, 35))
        x = np.stack([peaky(rng, T, V, pool) for _ in sub]) if T else np.zeros((len(sub), 0, V), np.float32)
        frames = rng.integers(0, T + 1, len(sub))
        recs = dv.step_records(dev(x), frames, sub)
        for r, s, f, row in zip(recs, sub, frames, x):
            check_record(r, orc[s].step(row[:f]), orc[s].status)
        if rng.random() < .5:
            s = int(rng.integers(n))
            what = rng.random()
            if what < .3:
                dv.reset([s]); orc[s].reset()
            elif what < .6:
                dv.reset_all([s]); orc[s].reset_all()
            else:
                own[s] = int(rng.integers(0, nsets))
                dv.assign([s], int(own[s])); orc[s] = oracle(sets[own[s]], c, cap)
    for s in range(n):
        assert dv.keywords_of(s) == own[s]
        assert dv.beams(s) == G.oracle_cur_hyps(orc[s].beam)


# ----------------------------------------------------------------------------------------------- the three fields
def test_threshold_is_the_sets():
    V = 20
    sets = [kwset([(3, 4)], .5), kwset([(3, 4)], .95)]
    dv, ids = spotter(2, V, sets)
    dv.assign([1], ids[1])
    x = rows(V, [0, 3, 3, 4, 4, 0, 0])
    orc = [oracle(s) for s in sets]
    want = [o.step(x) for o in orc]
    assert [w["state"] for w in want] == [1, 0]
    recs = step_all(dv, [x, x], [0, 1])
    for r, w in zip(recs, want):
        check_record(r, w)
    assert list(recs["state"]) == [1, 0]


def test_token_set_is_the_sets():
    V = 33
    sets = [kwset([(3, 4)], 2.0), kwset([(3, 4)], 2.0, tokenset=[0, 3, 4, 5, 32])]
    dv, ids = spotter(2, V, sets)
    dv.assign([1], ids[1])
    x = rows(V, [0, 3, 5, 5, 4, 32, 0, 3, 4])
    orc = [oracle(s) for s in sets]
    want = [o.step(x) for o in orc]
    recs = step_all(dv, [x, x], [0, 1])
    for s in range(2):
        check_record(recs[s], want[s])
        assert dv.beams(s) == G.oracle_cur_hyps(orc[s].beam)
    assert dv.beams(0) != dv.beams(1)
    assert any(5 in p or 32 in p for p, *_ in dv.beams(1)) and not any(5 in p or 32 in p for p, *_ in dv.beams(0))


def test_keyword_index_is_relative_to_the_set():
    V = 20
    sets = [kwset([(9,)], 0.0), kwset([(7, 8), (3, 4)], 0.0), kwset([(3, 4)], 0.0)]
    dv, ids = spotter(3, V, sets)
    dv.assign([1], ids[1])
    dv.assign([2], ids[2])
    x = rows(V, [0, 3, 3, 4, 0])
    orc = [oracle(s) for s in sets]
    recs = step_all(dv, [x, x, x], [0, 1, 2])
    for s in range(3):
        check_record(recs[s], orc[s].step(x))
    assert [int(k) for k in recs["keyword"]] == [-1, 1, 0] and list(recs["state"]) == [0, 1, 1]
    named = ctc.StreamingKeywordSpotter(2, {"zero": (9,)}, 0.0, min_frames=0, vocab=V)
    named.assign([1], named.add_keywords({"first": (7, 8), "second": (3, 4)}))
    got = named.step(dev(np.stack([x, x])))
    assert got[0]["keyword"] is None and got[1]["keyword"] == "second" and got[1]["state"] == 1


# ----------------------------------------------------------------------------------------------- assign, reset
def test_assign_is_reset_all_and_resets_keep_the_set():
    V = 20
    sets = [kwset([(3, 4)], 0.0), kwset([(7, 8), (3, 4)], 0.0)]
    dv, ids = spotter(2, V, sets)
    o = oracle(sets[0])
    a, b = rows(V, [0, 3, 3, 4, 4, 0]), rows(V, [0, 0, 3, 4])
    r = step_all(dv, [a], [0])[0]
    check_record(r, o.step(a))
    assert r["state"] == 1 and (r["start"], r["end"]) == (1, 3)          # a past activation ...
    r = step_all(dv, [b], [0])[0]
    check_record(r, o.step(b))
    assert r["state"] == 0 and r["start"] == 8                            # ... and carried frames
    dv.assign([0], ids[1])
    o = oracle(sets[1])
    r = step_all(dv, [a], [0])[0]
    check_record(r, o.step(a))
    assert r["state"] == 1 and r["keyword"] == 1 and (r["start"], r["end"]) == (1, 3)      # frame numbers from 0 again
    lib, h = dv._hd.lib, dv._hd.h
    for op in ("reset", "reset_all"):
        getattr(dv, op)([0]); getattr(o, op)()
        assert dv.keywords_of(0) == ids[1] and lib.wekws_hip_ctc_kws_stream_set(h, 0) == ids[1]
        r = step_all(dv, [b], [0])[0]
        check_record(r, o.step(b))
        assert r["keyword"] == 1
    assert lib.wekws_hip_ctc_kws_stream_set(h, 1) == 0 and lib.wekws_hip_ctc_kws_stream_set(h, 2) == -1


def test_drop_and_reuse_shows_only_the_new_set():
    V = 33
    sets = [kwset([(9,)], 0.0), kwset([(3, 4)], 0.0), kwset([(1, 2)], 0.3)]
    dv, ids = spotter(2, V, sets)
    dv.assign([0], ids[1])
    o = oracle(sets[1])
    x = rows(V, [0, 3, 4, 4, 0, 5, 6, 32, 0])
    with pytest.raises(_capi.HipLibraryError, match="in use"):
        dv.drop_keywords(ids[1])
    with pytest.raises(ValueError):
        dv.drop_keywords(0)
    assert dv.keywords_of(0) == ids[1]
    check_record(step_all(dv, [x], [0])[0], o.step(x))                     # the refusal changed nothing
    dv.assign([0], 0)
    dv.drop_keywords(ids[1])
    new = kwset([(5, 6)], 0.95, tokenset=[0, 5, 6, 32])                  # (the old threshold would activate: hit score 0.9)
    sid = dv.add_keywords(new["keywords"], new["threshold"], new["tokenset"])
    assert sid == ids[1]                                                    # the lowest free id
    dv.assign([0], sid)
    o = oracle(new)
    r = step_all(dv, [x], [0])[0]
    check_record(r, o.step(x))
    assert r["keyword"] == 0 and (r["start"], r["end"]) == (5, 6) and r["state"] == 0
    assert dv.beams(0) == G.oracle_cur_hyps(o.beam)
    assert any(32 in p for p, *_ in dv.beams(0)) and not any(3 in p or 4 in p for p, *_ in dv.beams(0))


# ----------------------------------------------------------------------------------------------- growth, scale
def test_tables_grow_under_load():
    """300 sets at V = 2599 registered in batches between steps: the record table, the keyword arena and the mask arena
    (82 words a set) all outgrow their first allocations several times while 12 streams keep decoding."""
    rng = np.random.default_rng(41)
    V, n = 2599, 12

    def one():
        return kwset([tuple(int(x) for x in rng.choice(np.arange(1, 30), int(rng.integers(1, 4)), replace=False))
                      for _ in range(int(rng.integers(1, 4)))], float(rng.uniform(0, .5)))

    sets = [one() for _ in range(4)]
    dv, ids = spotter(n, V, sets)
    own = [s % 4 for s in range(n)]
    for i in range(1, 4):
        dv.assign([s for s in range(n) if own[s] == i], ids[i])
    orc = [oracle(sets[own[s]]) for s in range(n)]
    pool = [k for s in sets for k in s["keywords"]]

    def step():
        x = np.stack([peaky(rng, 8, V, pool) for _ in range(n)])
        for r, s in zip(dv.step_records(dev(x)), range(n)):
            check_record(r, orc[s].step(x[s]))

    step()
    for _ in range(6):
        for _ in range(50):
            sets.append(one())
            ids.append(dv.add_keywords(sets[-1]["keywords"], sets[-1]["threshold"]))
        step()
    assert ids == list(range(304))
    for s in range(n):
        assert dv.beams(s) == G.oracle_cur_hyps(orc[s].beam)
    # the last sets
    last = list(range(304 - n, 304))
    for s in range(n):
        dv.assign([s], last[s])
        own[s] = last[s]
        orc[s] = oracle(sets[last[s]])
    pool = [k for i in last for k in sets[i]["keywords"]]
    step()
    step()
    for s in range(n):
        assert dv.beams(s) == G.oracle_cur_hyps(orc[s].beam)


def test_4096_streams_over_64_sets_sampled_and_permutation_invariant():
    rng = np.random.default_rng(8)
    V, n, T, nsets = 300, 4096, 4, 64
    sets = [kwset([(3 + k % 9, 4 + k % 11)] + ([(5 + k % 7,)] if k % 3 == 0 else []), .05 + .005 * k) for k in range(nsets)]
    pool = [k for s in sets for k in s["keywords"]]
    c = dict(CFG, min_frames=1, max_frames=80, interval_frames=3)
    a, ids = spotter(n, V, sets, c)
    b, _ = spotter(n, V, sets, c)
    for i in range(1, nsets):
        a.assign(list(range(i, n, nsets)), ids[i])
        b.assign(list(range(i, n, nsets)), ids[i])
    pick = rng.choice(n, 64, replace=False)
    orc = {int(s): oracle(sets[int(s) % nsets], c) for s in pick}
    for _ in range(3):
        x = np.stack([peaky(rng, T, V, pool) for _ in range(n)])
        xd = dev(x)
        ra = a.step_records(xd)
        perm = rng.permutation(n)
        rb = b.step_records(xd[torch.from_numpy(perm).cuda()], None, perm)
        inv = np.empty(n, np.int64)
        inv[perm] = np.arange(n)
        assert ra.tobytes() == rb[inv].tobytes()
        for s in pick:
            check_record(ra[s], orc[int(s)].step(x[s]))
    for s in pick[:8]:
        assert a.beams(int(s)) == b.beams(int(s)) == G.oracle_cur_hyps(orc[int(s)].beam)


def test_streams_left_in_set_0_are_untouched():
    rng = np.random.default_rng(9)
    V, n = 300, 12
    sets = [kwset([(3, 4, 5), (3, 6)], .2), kwset([(3, 6), (7,)], .1), kwset([], .3), kwset([(4, 5)], .0, tokenset=[0, 4, 5, 9])]
    c = dict(CFG, min_frames=2, interval_frames=20)
    plain, _ = spotter(n, V, sets[:1], c)
    multi, ids = spotter(n, V, sets, c)
    for i in (1, 2, 3):
        multi.assign([2 * i, 2 * i + 1], ids[i])
    stay = [0, 1, 8, 9, 10, 11]
    pool = [k for s in sets for k in s["keywords"]]
    for k in range(4):
        x = np.stack([peaky(rng, 20, V, pool) for _ in range(n)])
        ra, rb = plain.step_records(dev(x)), multi.step_records(dev(x))
        assert ra[stay].tobytes() == rb[stay].tobytes()
        if k == 1:
            multi.assign([2], multi.add_keywords([(8, 9)]))        # registering and assigning between steps
            multi.assign([3], 0)
            multi.drop_keywords(ids[1])
    for s in stay:
        assert plain.beams(s) == multi.beams(s)


# ----------------------------------------------------------------------------------------------- offline
def test_keyword_search_sets_against_keyword_search():
    rng = np.random.default_rng(12)
    V, B, T = 300, 16, 40
    lists = [[(3, 4), (5, 6, 7)], [(5, 6, 7)], [(8,), (3, 4), (9, 10)]]
    pool = [k for ks in lists for k in ks]
    x = np.stack([peaky(rng, T, V, pool) for _ in range(B)])
    lengths = rng.integers(1, T + 1, B)
    lengths[[2, 11]] = 0
    which = rng.integers(0, 3, B)
    which[:3] = [0, 1, 2]
    got = ctc.keyword_search_sets(dev(x), lengths, lists, which)
    for b in range(B):
        kws = lists[which[b]]
        k, score, start, end, _, _ = R.keyword_search(x[b, :lengths[b]], kws, 3, 20, R.default_tokenset(kws))
        assert got[b] == (k, score, start, end)
    for i, kws in enumerate(lists):
        sel = np.flatnonzero(which == i)
        assert ctc.keyword_search(dev(x[sel]), lengths[sel], kws) == [got[b] for b in sel]
    assert len({g[0] for g in got}) > 1
    named = ctc.keyword_search_sets(dev(x), lengths, [{"a": (3, 4), "b": (5, 6, 7)}, {"c": (5, 6, 7)}, lists[2]], which)
    for b in range(B):
        want = got[b][0] if got[b][0] is None or which[b] == 2 else [["a", "b"], ["c"]][which[b]][got[b][0]]
        assert named[b] == (want,) + got[b][1:]
    with pytest.raises(ValueError):
        ctc.keyword_search_sets(dev(x), lengths, lists, [3] * B)
    lib = _capi.load()
    hd = ctc._Handle(0, V, lists[0], None, 3, 20)
    res = torch.empty((1, 32), dtype=torch.uint8, device="cuda")
    bad = np.array([4], np.int32)
    assert lib.wekws_hip_ctc_kws_search_sets(hd.h, dev(x[:1]).data_ptr(), 1, T, None, bad.ctypes.data, res.data_ptr(), None, None) == -1
    assert "not registered" in _capi.last_error()


# ----------------------------------------------------------------------------------------------- errors
def test_refused_set_operations_change_nothing():
    V = 20
    dv, ids = spotter(3, V, [kwset([(3, 4)], 0.0), kwset([(5,)], 0.0)])
    hd = dv._hd
    for kws, ts in (([(3, 20)], None), ([()], None), ([(3,)], [0, 20])):
        with pytest.raises(_capi.HipLibraryError):
            hd.add_set(kws, ts, 0.5, 0)
    for streams, sid in (([0, 0], 1), ([3], 1), ([-1], 1)):
        with pytest.raises(ValueError):
            dv.assign(streams, sid)
    with pytest.raises(ValueError):
        dv.assign([0], 2)
    with pytest.raises(_capi.HipLibraryError, match="not registered"):
        hd.assign([0, 1], [1, 2], 0)
    with pytest.raises(_capi.HipLibraryError, match="twice"):
        hd.assign([1, 1], [1, 1], 0)
    assert [dv._hd.lib.wekws_hip_ctc_kws_stream_set(hd.h, s) for s in range(3)] == [0, 0, 0]
    assert dv.add_keywords([(6,)]) == 2                                     # the refused adds took no id
    x = rows(V, [0, 3, 4, 0])
    o = oracle(kwset([(3, 4)], 0.0))
    check_record(step_all(dv, [x], [1])[0], o.step(x))


# ----------------------------------------------------------------------------------------------- end to end, neighbours
def test_model_in_the_loop_two_keyword_lists():
    """PCM chunks of 8 streams through a synthetic CTC model: streams of two users' keyword lists in ONE spotter against one
    plain spotter per list; a stream moved to the other list mid-way is a fresh session of the other object."""
    from tests.test_hip_parity import build
    from wekws_amd import pack
    from wekws_amd.stream import BatchedKeyWordSpotter
    from wekws_amd.utils import synth
    cfg = dict(synth.MODEL_CONFIGS["ds_tcn_h64_ctc20"])
    model = build(cfg, synth.synth_state_dict(pack.model_spec(cfg), 5))
    # (tokens 3, 16 and 17 are among those this model's posteriors on this PCM activate: the names below do get used)
    A, B = {"a0": (3,), "a1": (16,)}, {"b0": (17,), "b1": (3,), "b2": (6, 7)}
    n = 8
    kw = dict(num_bins=40, window="hamming", max_chunk=4000, min_frames=0, max_frames=40)
    multi = BatchedKeyWordSpotter(model, {"unused": (1,)}, 0.0, n, **kw)
    sa, sb = multi.add_keywords(A), multi.add_keywords(B)
    assert (sa, sb) == (1, 2)
    multi.set_keywords(sa, [0, 1, 2, 3])
    multi.set_keywords(sb, [4, 5, 6, 7])
    plain = {sa: BatchedKeyWordSpotter(model, A, 0.0, n, **kw), sb: BatchedKeyWordSpotter(model, B, 0.0, n, **kw)}
    own = [sa] * 4 + [sb] * 4
    rng = np.random.default_rng(21)
    fired = set()
    for call in range(6):
        if call == 3:
            multi.set_keywords(sb, [2])
            own[2] = sb
            plain[sb].reset_all([2])
            assert multi.spotter.keywords_of(2) == sb and multi.frontend.counts(2) == (0, -1, 0, 0)
        chunks = [rng.integers(-12000, 12000, size=int(rng.choice([800, 1600, 2399, 3200])), dtype=np.int16) for _ in range(n)]
        got = multi.forward(chunks)
        want = {i: p.forward(chunks) for i, p in plain.items()}
        for s in range(n):
            assert got[s] == want[own[s]][s], (call, s)
            if got[s].get("state") == 1:
                fired.add(got[s]["keyword"])
    assert fired & set(A) and fired & set(B), fired               # hits were named from both lists
    multi.set_keywords(0, [2])
    multi.set_keywords(sa, [4, 5, 6, 7])
    multi.drop_keywords(sb)
    assert multi.add_keywords({"c": (9,)}) == sb


def test_beside_a_model_forward_on_another_stream():
    from wekws_amd.model.kws_model import init_model
    from wekws_amd.utils import synth
    from wekws_amd import pack
    cfg = synth.MODEL_CONFIGS["ds_tcn_h256_ctc"]
    m = init_model(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(pack.model_spec(cfg), 3).items()})
    m = m.cuda().eval()
    rng = np.random.default_rng(11)
    lists = [[(3, 4), (5, 6, 7)], [(5, 6, 7), (3,)], [(4,)], []]
    pool = [k for ks in lists for k in ks]
    x = np.stack([peaky(rng, 98, 2599, pool) for _ in range(256)])
    which = np.arange(256) % 4
    alone = ctc.keyword_search_sets(dev(x), None, lists, which)
    feats = torch.randn(512, 98, 40, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(3):
            m.forward_softmax(feats)
    together = ctc.keyword_search_sets(dev(x), None, lists, which)
    torch.cuda.synchronize()
    assert alone == together
    assert len({a[0] for a in alone}) > 1
