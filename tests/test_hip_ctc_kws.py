"""GPU: the on-device CTC prefix beam search and keyword detection (wekws_amd.ctc, csrc/ctc_kws.hip.h) against the
reference's own results (tests/golden/ctc_kws_golden.npz) and against the host restatement (tests/ctc_kws_ref.py) --
beams, pb / pnb, node records and hit scores compared as float64 bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ctc_kws_golden as G
from tests import ctc_kws_ref as R
from wekws_amd import _capi, ctc

pytestmark = pytest.mark.gpu

Z, META = G.load()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def check_record(rec, ref, status=0):
    """A device result record against the oracle's step record (None = the reference's `{}`: no frames, nothing changed;
    the record still carries the stream's sticky status)."""
    if ref is None:
        assert rec["valid"] == 0 and rec["status"] == status
        return
    assert rec["status"] == ref["status"]
    if ref["status"]:
        return
    assert rec["valid"] == 1 and rec["state"] == ref["state"]
    assert rec["keyword"] == (-1 if ref["hit"] is None else ref["hit"])
    assert (rec["start"], rec["end"]) == (ref["start"], ref["end"])
    assert np.float64(rec["score"]).tobytes() == np.float64(ref["score"]).tobytes()


def spotter_pair(c, n, **kw):
    dv = ctc.StreamingKeywordSpotter(n, c["keywords"], c["threshold"], c["min_frames"], c["max_frames"],
                                     c["interval_frames"], c["score_beam"], c["path_beam"], c["downsampling"], **kw)
    orc = [R.Spotter(c["keywords"], c["threshold"], c["min_frames"], c["max_frames"], c["interval_frames"], c["score_beam"],
                     c["path_beam"], c["downsampling"], capacity=kw.get("prefix_capacity")) for _ in range(n)]
    return dv, orc


# ----------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("case", META["offline"], ids=lambda c: c["name"])
def test_golden_offline_bit_identical(case):
    probs = Z[f"off/{case['name']}"]
    kws = [tuple(k) for k in case["keywords"]]
    ts = None if case["tokenset"] is None else set(case["tokenset"])
    beams = ctc.ctc_prefix_beam_search(dev(probs), case["lengths"], ts, case["score_beam"], case["path_beam"])
    hits = ctc.keyword_search(dev(probs), case["lengths"], kws, case["score_beam"], case["path_beam"]) if ts is not None else None
    for b, exp in enumerate(case["expect"]):
        got = [(p, s, [(n["token"], n["frame"], n["prob"]) for n in nodes]) for p, s, nodes in beams[b]]
        assert got == G.beam_expect(exp["beam"])
        if hits is not None:
            k, score, start, end = hits[b]
            assert (k, start, end) == (exp["hit"], exp["start"], exp["end"])
            assert score == G.fx(exp["score"])


@pytest.mark.parametrize("case", META["stream"], ids=lambda c: c["name"])
def test_golden_stream_bit_identical(case):
    c = case["config"]
    sp = ctc.StreamingKeywordSpotter(1, c["keywords"], c["threshold"], c["min_frames"], c["max_frames"], c["interval_frames"],
                                     c["score_beam"], c["path_beam"], c["downsampling"])
    i = 0
    for st in case["steps"]:
        if st["op"] != "chunk":
            getattr(sp, st["op"])([0])
            continue
        x = Z[f"str/{case['name']}/{i}"]
        i += 1
        if sp.vocab is None and x.shape[0] == 0:
            sp._create(x.shape[1])
        got = sp.step(dev(x[None]))[0]
        exp = st["result"]
        assert set(got) == set(exp)
        for key in exp:
            e = G.fx(exp[key]) if isinstance(exp[key], str) and key != "keyword" else exp[key]
            if key == "keyword" and e is not None:
                e = int(e[2:])
            assert got[key] == e, key
        assert sp.beams(0) == G.cur_hyps_expect(st["beam"])


# ----------------------------------------------------------------------------------------------- fuzz vs the oracle
def peaky(rng, T, V, kws):
    x = rng.normal(0, rng.uniform(.5, 2), (T, V)).astype(np.float32)
    t = 0
    while t < T:
        if rng.random() < .5:
            for tok in kws[rng.integers(len(kws))]:
                n = int(rng.integers(1, 5))
                x[t:t + n, tok] += rng.uniform(3, 8)
                t += n
        else:
            n = int(rng.integers(2, 10))
            x[t:t + n, 0] += rng.uniform(3, 8)
            t += n
    x = x - x.max(1, keepdims=True)
    e = np.exp(x)
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("cap", [None, 12])
@pytest.mark.parametrize("seed", range(6))
def test_fuzz_streams_against_oracle(seed, cap):
    """Random peaky posteriors, chunkings, stream subsets and resets; a small prefix capacity also compacts the node
    pool every few frames and fails streams whose prefix outgrows it, exactly where the oracle does."""
    rng = np.random.default_rng(100 + seed)
    V = int(rng.choice([20, 300, 2599]))
    kws = [tuple(int(x) for x in rng.choice(np.arange(1, min(V, 30)), int(rng.integers(1, 4)), replace=False))
           for _ in range(int(rng.integers(1, 4)))]
    c = dict(keywords=kws, threshold=float(rng.uniform(0, .7)), min_frames=int(rng.integers(0, 8)),
             max_frames=int(rng.integers(20, 120)), interval_frames=int(rng.integers(5, 60)),
             score_beam=int(rng.integers(1, 9)), path_beam=int(rng.choice([1, 4, 20, 33, 64])),
             downsampling=int(rng.choice([1, 3])))
    n = 12
    dv, orc = spotter_pair(c, n, vocab=V, prefix_capacity=cap)
    for _ in range(10 if cap is None else 30):
        sub = rng.permutation(n)[:int(rng.integers(1, n + 1))]
        T = int(rng.integers(0, 35))
        x = np.stack([peaky(rng, T, V, kws) for _ in sub]) if T else np.zeros((len(sub), 0, V), np.float32)
        frames = rng.integers(0, T + 1, len(sub))
        recs = dv.step_records(dev(x), frames, sub)
        for r, s, f, row in zip(recs, sub, frames, x):
            check_record(r, orc[s].step(row[:f]), orc[s].status)
        if rng.random() < .3:
            s = int(rng.integers(n))
            if rng.random() < .5:
                dv.reset([s]); orc[s].reset()
            else:
                dv.reset_all([s]); orc[s].reset_all()
    for s in range(n):
        assert dv.beams(s) == G.oracle_cur_hyps(orc[s].beam)


@pytest.mark.parametrize("seed", range(4))
def test_fuzz_offline_against_oracle(seed):
    rng = np.random.default_rng(200 + seed)
    V = int(rng.choice([20, 300, 2599]))
    sb, pb = int(rng.integers(1, 9)), int(rng.choice([1, 5, 20, 64]))
    kws = [tuple(int(x) for x in rng.choice(np.arange(1, min(V, 30)), int(rng.integers(1, 4)), replace=False)) for _ in range(2)]
    B, T = 16, int(rng.integers(1, 100))
    x = np.stack([peaky(rng, T, V, kws) for _ in range(B)])
    lengths = rng.integers(0, T + 1, B)
    ts = R.default_tokenset(kws) if seed % 2 else None
    beams = ctc.ctc_prefix_beam_search(dev(x), lengths, ts, sb, pb)
    hits = ctc.keyword_search(dev(x), lengths, kws, sb, pb)
    for b in range(B):
        beam, st = R.prefix_beam_search(x[b, :lengths[b]], sb, pb, ts)
        assert [(p, s, [(n["token"], n["frame"], n["prob"]) for n in nodes]) for p, s, nodes in beams[b]] == G.oracle_beam(beam)
        k, score, start, end, _, _ = R.keyword_search(x[b, :lengths[b]], kws, sb, pb, R.default_tokenset(kws))
        assert hits[b] == (k, score, start, end)


def test_4096_streams_sampled_and_permutation_invariant():
    rng = np.random.default_rng(7)
    V, n, T = 300, 4096, 30
    kws = [(3, 4, 5), (3, 6)]
    c = dict(keywords=kws, threshold=.2, min_frames=2, max_frames=80, interval_frames=20, score_beam=3, path_beam=20,
             downsampling=1)
    a, _ = spotter_pair(c, n, vocab=V)
    b, _ = spotter_pair(c, n, vocab=V)
    pick = rng.choice(n, 64, replace=False)
    orc = {int(s): R.Spotter(kws, .2, 2, 80, 20) for s in pick}
    for _ in range(3):
        x = np.stack([peaky(rng, T, V, kws) for _ in range(n)])
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


# ----------------------------------------------------------------------------------------------- deviations, errors
def test_topk_ties_go_lower_index_first():
    row = np.array([[.1, .3, .3, .05, .3]], np.float32)
    beams = ctc.ctc_prefix_beam_search(dev(row[None]), [1], None, 3, 20)
    assert [p for p, _, _ in beams[0]] == [(1,), (2,), (4,)]
    beam, _ = R.prefix_beam_search(row, 3, 20, None)
    assert [p for p, _, _ in beams[0]] == [h.prefix for h in beam]


def test_nan_row_skipped_inf_row_fails_its_stream_only():
    x = np.full((2, 4, 5), .01, np.float32)
    x[:, :, 1] = .96
    x[0, 1, :] = np.nan                                # skipped frame: same as the reference
    x[1, 2, 3] = np.inf
    sp = ctc.StreamingKeywordSpotter(3, [(1,)], 2.0)
    r = sp.step_records(dev(np.concatenate([x, x[:1]])))
    assert list(r["status"]) == [0, R.EINVAL, 0] and sp.status(1) == R.EINVAL and sp.status(0) == 0
    o = R.Spotter([(1,)], 2.0)
    check_record(r[0], o.step(x[0]))
    assert sp.step(dev(x[:1]), None, [1]) == [{"status": R.EINVAL}]
    sp.reset([1])
    assert sp.status(1) == 0
    with pytest.raises(ValueError):
        ctc.keyword_search(dev(x), None, [(1,)])


def test_prefix_capacity_overflow_is_reported_not_truncated():
    x = np.full((1, 12, 8), .01, np.float32)
    for t in range(12):
        x[0, t, 1 + t % 6] = .9                         # a new token every frame
    sp = ctc.StreamingKeywordSpotter(2, [(1, 2, 3, 4, 5, 6)], 2.0, max_frames=1000, prefix_capacity=5)
    r = sp.step_records(dev(x))
    assert r["status"][0] == R.ECAPACITY
    before = sp.beams(0)
    assert max(len(p) for p, *_ in before) <= 5 and len(before[0][0]) == 5
    o = R.Spotter([(1, 2, 3, 4, 5, 6)], 2.0, max_frames=1000, capacity=5)
    assert o.step(x[0])["status"] == R.ECAPACITY and G.oracle_cur_hyps(o.beam) == before
    assert sp.step_records(dev(x[:, :1]))["status"][0] == R.ECAPACITY      # sticky


def test_argument_errors_are_rejected():
    lib = _capi.load()
    h = C.c_void_p()
    for kw in (dict(score_beam=9), dict(vocab=0), dict(path_beam=65), dict(prefix_capacity=0)):
        d = _capi.CtcKwsDesc(vocab=10, score_beam=3, path_beam=20, max_streams=1, prefix_capacity=8, downsampling=1)
        for k, v in kw.items():
            setattr(d, k, v)
        assert lib.wekws_hip_ctc_kws_create(C.byref(d), C.byref(h)) == -1 and not h.value
        assert _capi.last_error()
    sp = ctc.StreamingKeywordSpotter(2, [(1,)], .5)
    with pytest.raises(ValueError):
        sp.step(dev(np.zeros((1, 3, 10))), None, [2])
    with pytest.raises(ValueError):
        sp.step(dev(np.zeros((2, 3, 10))), None, [1, 1])
    with pytest.raises(ValueError):
        ctc.ctc_prefix_beam_search(dev(np.zeros((1, 3, 0))), None)
    # a bad id inside the device array is reported on its row, and no stream is touched
    ids = torch.tensor([0, 7], dtype=torch.int32, device="cuda")
    res = torch.empty((2, 32), dtype=torch.uint8, device="cuda")
    x = dev(np.full((2, 2, 10), .1))
    _capi.check(sp._hd.lib.wekws_hip_ctc_kws_step(sp._hd.h, x.data_ptr(), 2, 2, ids.data_ptr(), None, res.data_ptr(), None),
                "step")
    r = ctc._results(res)
    assert list(r["status"]) == [0, R.EINVAL]


def test_beside_a_model_forward_on_another_stream():
    from wekws_amd.model.kws_model import init_model
    from wekws_amd.utils import synth
    from wekws_amd import pack
    cfg = synth.MODEL_CONFIGS["ds_tcn_h256_ctc"]
    m = init_model(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(pack.model_spec(cfg), 3).items()})
    m = m.cuda().eval()
    rng = np.random.default_rng(11)
    kws = [(3, 4), (5, 6, 7)]
    x = np.stack([peaky(rng, 98, 2599, kws) for _ in range(256)])
    alone = ctc.keyword_search(dev(x), None, kws)
    feats = torch.randn(512, 98, 40, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(3):
            m.forward_softmax(feats)
    together = ctc.keyword_search(dev(x), None, kws)
    torch.cuda.synchronize()
    assert alone == together


def test_end_to_end_ds_tcn_ctc_streaming():
    """ds_tcn_h256_ctc's forward_softmax in 30-frame chunks, then the spotter: the same result dicts as the oracle fed
    the same posteriors."""
    from wekws_amd.model.kws_model import init_model
    from wekws_amd.utils import synth
    from wekws_amd import pack
    cfg = synth.MODEL_CONFIGS["ds_tcn_h256_ctc"]
    m = init_model(cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(pack.model_spec(cfg), 1).items()})
    m = m.cuda().eval()
    B, T = 8, 150
    feats = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (B, T, 40)).astype(np.float32)).cuda()
    kws = {"k0": (1, 2), "k1": (3,)}
    sp = ctc.StreamingKeywordSpotter(B, kws, 0.0, min_frames=0)
    orc = [R.Spotter(list(kws.values()), 0.0, min_frames=0) for _ in range(B)]
    cache = torch.zeros(0, 0, 0)
    for t in range(0, T, 30):
        probs, cache = m.forward_softmax(feats[:, t:t + 30], cache)
        got = sp.step(probs)
        host = probs.cpu().numpy()
        for b in range(B):
            assert got[b] == R.as_result_dict(orc[b].step(host[b]), list(kws))
