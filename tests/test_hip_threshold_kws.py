"""GPU: the streaming threshold detector (wekws_amd.det.StreamingThresholdSpotter over wekws_hip_threshold_kws_*): the alarm scan
of compute_det.py:89-96 carried across chunks.  For any split of a score sequence into chunks the fired frames are those of ONE
scan over the whole sequence -- written out below, and counted by oracle/det_oracle.py::false_alarms."""
import numpy as np
import pytest
import torch

from oracle import det_oracle
from wekws_amd.det import StreamingThresholdSpotter

pytestmark = pytest.mark.gpu

STREAMS, T = 7, 230
TH = np.float32(0.7)                         # a threshold that IS a float32: a score can equal it exactly


def scores(K, seed=0):
    """(STREAMS, T, K) seeded scores in [0, 0.75), about one frame in eight at or above the threshold, with the planted cases."""
    rng = np.random.default_rng(seed)
    s = (np.sqrt(rng.random((STREAMS, T, K))) * 0.75).astype(np.float32)
    below = np.nextafter(TH, np.float32(0))
    s[0, :, 0] = 0.1
    s[0, 29, 0] = 0.9            # stream 0's first chunks are 30 frames (chunk_plan): a hit on the LAST frame of a chunk ...
    s[0, 30:90, 0] = 0.95        # ... whose skip spans the following chunks: with window_shift 50 the next hit is frame 79
    s[1, :, 0] = 0.1
    s[1, 40, 0] = TH             # exactly the threshold: fires
    s[1, 120, 0] = below         # one ulp below: does not
    s[1, 121, 0] = np.nan        # never fires, and the maximum ignores it
    s[2, 5, K - 1] = np.nan
    s[3, :, 0] = below           # a stream that never fires
    s[4, :, K - 1] = 0.99        # one that fires as often as the window allows
    return s


def chunk_plan(seed, first30=True):
    """Calls [(stream, chunk length)]: lengths 0 .. 30, subsets of the streams in permuted order, until every stream is through.
    Stream 0 starts with chunks of 30, 3, 0, 7 frames (the planted hit on a chunk's last frame, a skip over more than three
    chunks)."""
    rng = np.random.default_rng(seed)
    todo = [T] * STREAMS
    fixed = {0: [30, 3, 0, 7]} if first30 else {}
    calls = []
    while any(todo):
        live = [s for s in range(STREAMS) if todo[s]]
        pick = [s for s in live if rng.random() < 0.7] or live[:1]
        pick = [pick[i] for i in rng.permutation(len(pick))]
        call = []
        for s in pick:
            n = fixed[s].pop(0) if fixed.get(s) else int(rng.integers(0, 31))
            n = min(n, todo[s])
            todo[s] -= n
            call.append((s, n))
        calls.append(call)
    return calls


def whole_scan(x, th, window_shift):
    """Fired frames of one scan over the whole sequence x (float32): compute_det.py:89-96."""
    hits, i = [], 0
    while i < len(x):
        if float(x[i]) >= th:
            hits.append(i)
            i += window_shift
        else:
            i += 1
    return hits


def run_chunked(spot, s, calls, check=None):
    """Feeds the calls; returns per stream and keyword the (frame, score) pairs of its hits, in the order they came."""
    K = s.shape[2]
    pos = [0] * STREAMS
    got = [[[] for _ in range(K)] for _ in range(STREAMS)]
    for call in calls:
        ids = [sid for sid, _ in call]
        ns = [n for _, n in call]
        cap = max(ns + [1])
        x = np.zeros((len(call), cap, K), np.float32)
        x[:] = 0.999                                            # rows past a count must not be read: they would all fire
        for b, (sid, n) in enumerate(call):
            x[b, :n] = s[sid, pos[sid]:pos[sid] + n]
            pos[sid] += n
        out = spot.step(torch.from_numpy(x).cuda(), frames=ns, streams=ids)
        for b, sid in enumerate(ids):
            assert [(h["frame"], h["keyword"]) for h in out[b]] == sorted((h["frame"], h["keyword"]) for h in out[b])
            for h in out[b]:
                k = spot.names.index(h["keyword"])
                assert pos[sid] - ns[b] <= h["frame"] < pos[sid]            # a hit lies in the chunk that was given
                assert h["time"] == h["frame"] * spot.resolution
                got[sid][k].append((h["frame"], np.float32(h["score"])))
        if check is not None:
            check(ids, pos)
    assert pos == [T] * STREAMS
    return got


@pytest.mark.parametrize("window_shift", [50, 7, 1])
@pytest.mark.parametrize("K", [1, 3])
def test_chunked_equals_whole(K, window_shift):
    s = scores(K)
    names = [f"k{k}" for k in range(K)]
    spot = StreamingThresholdSpotter(STREAMS, names, float(TH), window_shift=window_shift)
    calls = chunk_plan(1)
    assert [n for c in calls for sid, n in c if sid == 0][:4] == [30, 3, 0, 7]
    assert any(n == 0 for c in calls for _, n in c) and any(len(c) < STREAMS for c in calls)
    got = run_chunked(spot, s, calls)
    fired = 0
    for sid in range(STREAMS):
        for k in range(K):
            want = whole_scan(s[sid, :, k], float(TH), window_shift)
            assert [a for a, _ in got[sid][k]] == want, (sid, k)
            assert all(np.array_equal(v, s[sid, a, k]) for a, v in got[sid][k]), (sid, k)
            assert len(want) == det_oracle.false_alarms(s[sid, :, k].tolist(), float(TH), window_shift), (sid, k)
            st = spot.state(sid, k)
            assert st["seen"] == T and st["resume"] == (want[-1] + window_shift if want else 0)
            fired += len(want)
    assert fired > 20
    # the planted cases
    h0, h1 = [a for a, _ in got[0][0]], [a for a, _ in got[1][0]]
    if window_shift == 50:
        assert h0 == [29, 79]                   # fired on the last frame of the first chunk; frames 30 .. 78 lie in later chunks
    elif window_shift == 7:
        assert h0[:3] == [29, 36, 43]
    else:
        assert h0 == list(range(29, 90))
    assert 40 in h1 and 120 not in h1 and 121 not in h1
    assert got[3][0] == []
    assert [a for a, _ in got[4][K - 1]] == list(range(0, T, window_shift))


def test_running_maximum_after_every_step():
    """best / best_frame are oracle.det_oracle.max_pool of the frames so far (first frame of a tie, NaN ignored), after every
    step, for the streams of the step and for those it left out."""
    K = 3
    s = scores(K, seed=3)
    s[5, 10, 1] = s[5, 60, 1] = 0.97            # a tie across chunks: the first frame stays
    s[6, :4, 2] = np.nan                        # a stream whose first chunk may be NaN alone
    spot = StreamingThresholdSpotter(STREAMS, ["a", "b", "c"], float(TH), window_shift=50)
    for sid in range(STREAMS):
        assert spot.best(sid) == ([-np.inf] * K, [-1] * K)

    def check(ids, pos):
        for sid in range(STREAMS):
            best, frame = spot.best(sid)
            clean = np.where(np.isnan(s[sid:sid + 1, :pos[sid]]), -np.inf, s[sid:sid + 1, :pos[sid]])
            mx, am = det_oracle.max_pool(clean)
            # (a prefix of NaN alone: the oracle's -inf at frame 0 is the detector's "nothing yet")
            am = np.where(np.isinf(mx), -1, am)
            assert np.array_equal(np.asarray(best, np.float32), mx[0]) and frame == am[0].tolist(), (sid, pos[sid])

    run_chunked(spot, s, chunk_plan(4, first30=False), check)
    assert spot.best(5)[1][1] == 10


def test_unlisted_streams_keep_their_state_and_reset_clears_the_named():
    K = 2
    s = scores(K, seed=5)
    spot = StreamingThresholdSpotter(STREAMS, ["a", "b"], float(TH), window_shift=7)
    x = torch.from_numpy(s[:, :40]).cuda()
    spot.step(x)
    before = [[spot.state(sid, k) for k in range(K)] for sid in range(STREAMS)]
    assert all(st["seen"] == 40 for row in before for st in row)
    spot.step(x[[2, 5]].contiguous(), streams=[5, 2], frames=[11, 0])
    for sid in range(STREAMS):
        for k in range(K):
            st = spot.state(sid, k)
            if sid == 5:
                assert st["seen"] == 51
            else:
                assert st == before[sid][k], (sid, k)            # left out, or given no frame
    spot.reset([1, 4])
    for sid in range(STREAMS):
        for k in range(K):
            st = spot.state(sid, k)
            if sid in (1, 4):
                assert st == dict(seen=0, resume=0, best_frame=-1, best=-np.inf)
            elif sid != 5:
                assert st == before[sid][k]
    # a reset stream scans from frame 0 again, with no skip pending
    out = spot.step(torch.from_numpy(s[4:5, :40]).cuda(), streams=[4])
    assert [h["frame"] for h in out[0] if h["keyword"] == "b"] == whole_scan(s[4, :40, 1], float(TH), 7) == list(range(0, 40, 7))
    spot.reset()
    assert all(spot.state(sid, k)["seen"] == 0 for sid in range(STREAMS) for k in range(K))


def test_per_keyword_thresholds():
    K = 3
    s = scores(K, seed=6)
    th = [0.3, float(TH), 0.74]
    spot = StreamingThresholdSpotter(STREAMS, ["a", "b", "c"], th, window_shift=7)
    got = run_chunked(spot, s, chunk_plan(7, first30=False))
    counts = []
    for sid in range(STREAMS):
        for k in range(K):
            want = whole_scan(s[sid, :, k], th[k], 7)
            assert [a for a, _ in got[sid][k]] == want, (sid, k)
            counts.append(len(want))
    assert len(set(counts)) > 3


def test_step_records_stay_on_the_device():
    """step_records returns device tensors of the documented shapes (hits ascending, -1 fill) and takes device frame counts."""
    s = scores(2, seed=8)
    spot = StreamingThresholdSpotter(STREAMS, ["a", "b"], float(TH), window_shift=7)
    x = torch.from_numpy(s[:, :23]).cuda()
    fr = torch.tensor([23, 0, 5, 23, 23, 1, 22], dtype=torch.int32, device="cuda")
    hf, hs, best, bf, status = spot.step_records(x, frames=fr)
    assert hf.shape == hs.shape == (STREAMS, 2, 4) and best.shape == bf.shape == (STREAMS, 2) and status.shape == (STREAMS,)
    assert all(t.is_cuda for t in (hf, hs, best, bf, status)) and not status.any()
    hf, hs = hf.cpu().numpy(), hs.cpu().numpy()
    for sid in range(STREAMS):
        for k in range(2):
            want = whole_scan(s[sid, :int(fr[sid]), k], float(TH), 7)
            assert hf[sid, k].tolist() == want + [-1] * (4 - len(want))
            assert np.array_equal(hs[sid, k, :len(want)], s[sid, want, k]) and not hs[sid, k, len(want):].any()
    assert bf.cpu().numpy()[1].tolist() == [-1, -1] and np.isneginf(best.cpu().numpy()[1]).all()


def test_python_refusals_reach_no_launch():
    spot = StreamingThresholdSpotter(4, ["a", "b"], 0.5)
    x = torch.zeros((3, 10, 2), device="cuda")
    before = [spot.state(sid, 0) for sid in range(4)]
    for kw in (dict(streams=[0, 1, 1]), dict(streams=[0, 1, 4]), dict(streams=[0, -1, 2]), dict(streams=[0, 1]),
               dict(frames=[10, 11, 0]), dict(frames=[10, -1, 0]), dict(frames=[10, 10])):
        with pytest.raises(ValueError):
            spot.step(x, **kw)
    with pytest.raises(ValueError):
        spot.step(torch.zeros((3, 10, 3), device="cuda"))           # another number of keywords
    with pytest.raises(ValueError):
        spot.step(torch.zeros((3, 10, 2)))                          # not on the device
    with pytest.raises(ValueError):
        spot.reset([0, 9])
    with pytest.raises(ValueError):
        spot.best(4)
    assert [spot.state(sid, 0) for sid in range(4)] == before
    assert spot.step(torch.zeros((0, 10, 2), device="cuda")) == []
    assert spot.step(torch.zeros((2, 0, 2), device="cuda")) == [[], []]
