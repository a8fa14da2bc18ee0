"""GPU: the streaming front end (wekws_amd.frontend.StreamingFrontEnd over wekws_hip_stream_frontend_*).

Every frame a stream produces is frame k of its whole signal -- samples [k S, k S + L) -- and the streaming kernel shares the
one-shot kernel's arithmetic, so the expected value of every output row is a GATHER from ``Fbank(...)(whole signal)`` with
the indices of the host restatement (tests/stream_frontend_ref.py, pinned against the live reference), bit for bit."""
import copy

import numpy as np
import pytest
import torch

from oracle import fbank_oracle, splice_oracle
from tests import stream_frontend_ref as sref
from tests.helpers import K_FBANK
from wekws_amd import _capi
from wekws_amd.frontend import Fbank, StreamingFrontEnd

pytestmark = pytest.mark.gpu

CHUNKS = [0, 1, 2, 159, 160, 161, 399, 400, 401, 4800]
FB = {  # name -> Fbank / StreamingFrontEnd keyword arguments
    "h40": dict(num_bins=40, window="hamming"),
    "p80": dict(num_bins=80, window="povey"),
    "h16_8k": dict(num_bins=16, window="hamming", sample_rate=8000, frame_length=200, frame_shift=80),
}
_cache = {}


def noise(streams, n, seed):
    return np.random.default_rng(seed).integers(-20000, 20000, size=(streams, n), dtype=np.int16)


def one_shot(fb, pcm, key=None):
    """(streams, T, F) features of the whole signals by the one-shot kernel; computed once per key."""
    if key is not None and key in _cache:
        return _cache[key]
    kw = FB[fb]
    out = Fbank(kw["num_bins"], kw.get("sample_rate", 16000), kw.get("frame_length"), kw.get("frame_shift"), kw["window"])(
        torch.from_numpy(pcm).cuda()).cpu().numpy()
    if key is not None:
        _cache[key] = out
    return out


def frame_geometry(fb):
    kw = FB[fb]
    return kw.get("frame_length", 400), kw.get("frame_shift", 160)


def schedule(rng, total, big=False, lo=0):
    """Chunk sizes that sum to `total`: the fixed sizes and random 1..3000 (big: every chunk well over 2 r frames)."""
    out, left = [], total
    while left > 0:
        if big:
            n = int(rng.integers(lo, 4801))
        else:
            n = int(rng.choice(CHUNKS)) if rng.random() < 0.5 else int(rng.integers(1, 3001))
        n = min(n, left)
        out.append(n)
        left -= n
    return out


class Driver:
    """Feeds per-stream schedules to a front end in calls that mix streams in different states, in permuted order and with
    some left out; checks every call against the restatement's gather from the one-shot features."""

    def __init__(self, fb, pcm, left=0, right=0, skip=1, max_chunk=4800, num_streams=None, feats=None):
        self.L, self.S = frame_geometry(fb)
        self.pcm = pcm
        self.n = pcm.shape[0] if num_streams is None else num_streams
        self.fe = StreamingFrontEnd(self.n, left=left, right=right, skip=skip, max_chunk=max_chunk, **FB[fb])
        self.refs = [sref.StreamRef(self.L, self.S, left, right, skip) for _ in range(self.n)]
        self.pos = [0] * self.n
        self.feats = feats
        self.rows = [[] for _ in range(self.n)]       # what each stream has delivered

    def safe(self, sid, n):
        """A size the reference accepts (only r = 1 can assert): whole frame shifts longer, or nothing."""
        left = self.pcm.shape[1] - self.pos[sid]
        while sref.is_marker(copy.deepcopy(self.refs[sid]).push(n), sref.ASSERT):
            n = n + self.S if n + self.S <= left else 0
        return n

    def call(self, ids, sizes, check=True):
        sizes = [self.safe(s, min(n, self.pcm.shape[1] - self.pos[s])) for s, n in zip(ids, sizes)]
        nmax = max(sizes + [0])
        host = np.zeros((len(ids), nmax), np.int16)
        for b, (s, n) in enumerate(zip(ids, sizes)):
            host[b, :n] = self.pcm[s, self.pos[s]:self.pos[s] + n]
            self.pos[s] += n
        feats, frames = self.fe.push(torch.from_numpy(host).cuda(), samples=sizes, streams=ids)
        feats = feats.cpu().numpy()
        for b, s in enumerate(ids):
            res = self.refs[s].push(sizes[b])
            if sref.is_marker(res, sref.HELD):
                assert frames[b] == -1, (s, sizes[b], frames[b])
                rows = 0
            else:
                assert frames[b] == res.shape[0], (s, sizes[b], frames[b], res.shape)
                rows = res.shape[0]
                if check and rows:
                    want = self.feats[s][res].reshape(rows, -1)
                    assert np.array_equal(feats[b, :rows].view(np.int32), want.view(np.int32)), (s, sizes[b], self.pos[s])
                self.rows[s].append(feats[b, :rows].copy())
            assert not feats[b, rows:].any(), (s, "rows past the count are zero")
            assert self.fe.counts(s)[:3] == self.refs[s].counts(), (s, self.fe.counts(s), self.refs[s].counts())
            assert self.fe.counts(s)[3] == self.refs[s].rows_total
        return feats, frames

    def run(self, rng, schedules):
        todo = [list(s) for s in schedules]
        calls = 0
        while any(todo):
            live = [s for s in range(len(todo)) if todo[s]]
            pick = [s for s in live if rng.random() < 0.7] or [live[0]]
            pick = [pick[i] for i in rng.permutation(len(pick))]
            self.call(pick, [todo[s].pop(0) for s in pick])
            calls += 1
        return calls

    def delivered(self, s):
        rows = self.rows[s]
        return np.concatenate(rows) if rows else np.zeros((0, self.fe.feat_dim), np.float32)


@pytest.mark.parametrize("fb", ["h40", "p80", "h16_8k"])
def test_frames_equal_the_one_shot_kernel(fb):
    """5 streams of 12,000 samples in chunks of 0 / 1 / 2 / 159 / 160 / 161 / 399 / 400 / 401 / 4800 / random: every produced
    frame k is Fbank(whole)[k] bit for bit (odd leftovers: the chunk side of a frame is pair-misaligned), counts are the plan's."""
    pcm = noise(5, 12000, 1)
    feats = one_shot(fb, pcm, (fb, "t1"))
    rng = np.random.default_rng(2)
    d = Driver(fb, pcm, feats=feats)
    scheds = [schedule(rng, 12000) for _ in range(5)]
    assert any(n % 2 for s in scheds for n in s)
    assert d.run(rng, scheds) > 5
    L, S = d.L, d.S
    for s in range(5):
        got = d.delivered(s)
        assert got.shape[0] == 1 + (12000 - L) // S                    # every frame of the signal, once
        assert np.array_equal(got.view(np.int32), feats[s].view(np.int32))
        assert d.fe.counts(s) == (12000 - got.shape[0] * S, -1, 0, got.shape[0])
    if fb == "p80":                                                    # ... and against the float64 evaluation at the tight bar
        for s in range(5):
            u = fbank_oracle.fbank_units(d.delivered(s), pcm[s].astype(np.float32), 80, 16000, 400, 160, 1)
            assert float(u.max()) <= K_FBANK, (s, float(u.max()))


CTX = [("p80", 2, 2, 3), ("h40", 1, 1, 1), ("h40", 3, 3, 2), ("h40", 0, 0, 3)]


@pytest.mark.parametrize("fb,left,right,skip", CTX)
def test_context_and_skip(fb, left, right, skip):
    """Rows are the restatement's indices gathered from the one-shot features, bit for bit: mixed schedules (held pushes, pushes
    of fewer than 2 r frames after a steady one), and big chunks, where the rows also equal splice_skip(one_shot)."""
    pcm = noise(5, 12000, 1)
    feats = one_shot(fb, pcm, (fb, "t1"))
    rng = np.random.default_rng(5)
    d = Driver(fb, pcm, left, right, skip, feats=feats)
    scheds = [schedule(rng, 12000) for _ in range(4)] + [[4800, 500, 4800, 480, 481, 939]]   # r = 2: 820 samples = 3 frames < 2 r
    d.run(rng, scheds)
    if (left, right) == (2, 2):
        assert d.refs[4].rows_total > 0
    # chunks of at least 2 r frames (and a whole frame): the concatenation is the one-shot splice
    d2 = Driver(fb, pcm, left, right, skip, feats=feats)
    lo = d2.S * (2 * right + 3)
    d2.run(rng, [schedule(rng, 12000, big=True, lo=lo) for _ in range(5)])
    want = splice_oracle.splice_skip(feats, left, right, skip)
    for s in range(5):
        got = d2.delivered(s)
        # (a last chunk cut short by the end of the signal may be held: the stream then lacks the one-shot's last rows)
        assert got.shape[0] >= want.shape[1] - (lo // d2.S + 2 * right) // skip - 1
        assert np.array_equal(got.view(np.int32), want[s, :got.shape[0]].view(np.int32)), s


def test_size_2048_streams():
    """2,048 streams x 3 pushes x 4,800 samples (61,440 frames per push) with context (2, 2) and skip 3 on 80 bins: bit-identical to
    the same streams pushed 8 at a time on a second handle; 16 sampled streams against the one-shot features.
    The fbank kernel's grid is capped at one resident round of 4-wave workgroups, one frame per wave (register-bound: four
    workgroups per CU at 128 registers, 256 CUs -- a few thousand frames in flight): 61,440 frame slots wrap it more than ten
    times, so the persistent walk over (row, frame slot) and its carries run."""
    streams, pushes, n = 2048, 3, 4800
    g = torch.Generator(device="cuda").manual_seed(4)
    pcm = torch.randint(-20000, 20000, (streams, pushes * n), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
    a = StreamingFrontEnd(streams, left=2, right=2, skip=3, max_chunk=n, **FB["p80"])
    b = StreamingFrontEnd(streams, left=2, right=2, skip=3, max_chunk=n, **FB["p80"])
    sample = np.random.default_rng(6).choice(streams, 16, replace=False)
    feats = one_shot("p80", pcm[torch.from_numpy(sample).cuda()].cpu().numpy())
    refs = [sref.StreamRef(400, 160, 2, 2, 3) for _ in sample]
    for p in range(pushes):
        chunk = pcm[:, p * n:(p + 1) * n].contiguous()
        fa, na = a.push(chunk)
        cap = fa.shape[1]
        fb_ = torch.zeros_like(fa)
        for s0 in range(0, streams, 8):
            f8, n8 = b.push(chunk[s0:s0 + 8], streams=range(s0, s0 + 8), capacity=cap)
            assert n8 == na[s0:s0 + 8]
            fb_[s0:s0 + 8] = f8
        assert torch.equal(fa.view(torch.int32), fb_.view(torch.int32)), p
        host = fa[torch.from_numpy(sample).cuda()].cpu().numpy()
        for i, s in enumerate(sample):
            res = refs[i].push(n)
            assert na[s] == res.shape[0]
            assert np.array_equal(host[i, :na[s]].view(np.int32), feats[i][res].reshape(na[s], -1).view(np.int32)), (p, s)


def test_back_to_back_pushes_equal_synchronised_ones():
    """Six pushes queued with no synchronise between them (more than the plan ring holds: it wraps) equal the same pushes with a
    synchronise after each."""
    streams, n = 512, 1600
    sizes = [1600, 1599, 801, 1600, 3, 1600]
    pcm = torch.from_numpy(noise(streams, sum(sizes), 8)).cuda()
    chunks, at = [], 0
    for k in sizes:
        chunks.append(pcm[:, at:at + k].contiguous())
        at += k
    out = {}
    for mode in ("sync", "queued"):
        fe = StreamingFrontEnd(streams, left=2, right=2, skip=3, max_chunk=n, **FB["p80"])
        cap = fe.max_frames(n)
        torch.cuda.synchronize()
        res = []
        for c in chunks:
            res.append(fe.push(c, capacity=cap))
            if mode == "sync":
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        out[mode] = res
    for (fs, ns), (fq, nq) in zip(out["sync"], out["queued"]):
        assert ns == nq
        assert torch.equal(fs.view(torch.int32), fq.view(torch.int32))
    assert any(max(ns) > 0 for _, ns in out["sync"])


def test_reset_restarts_the_streams_it_names():
    pcm = noise(6, 12000, 9)
    feats = one_shot("p80", pcm, ("p80", "t5"))
    d = Driver("p80", pcm, 2, 2, 3, feats=feats)
    ids = list(range(6))
    d.call(ids, [4800] * 6)
    d.call(ids, [1001] * 6)
    assert d.fe.counts(2)[:3] == (361, 4, 1)
    before = [d.fe.counts(s) for s in ids]
    d.fe.reset([1, 4])
    for s in ids:
        assert d.fe.counts(s) == ((0, -1, 0, 0) if s in (1, 4) else before[s])
    # the reset streams start over on a signal of their own: their samples from here on
    pcm2 = pcm.copy()
    for s in (1, 4):
        pcm2[s, :12000 - 5801] = pcm[s, 5801:]
        d.refs[s].reset()
        d.pos[s] = 0
    d.pcm = pcm2
    feats2 = feats.copy()
    fresh = one_shot("p80", pcm2[[1, 4]])
    feats2[1], feats2[4] = fresh[0], fresh[1]
    d.feats = feats2
    out, frames = d.call(ids, [3000] * 6)      # checked row by row: streams 1 and 4 get the first-chunk replicate pad, phase 0
    r = d.refs[1]
    assert frames[1] == frames[4] and frames[1] != frames[0]
    assert np.array_equal(out[1, 0, :80], out[1, 0, 80:160]) and np.array_equal(out[1, 0, :80], out[1, 0, 160:240])   # replicate pad
    d.call(ids, [1500] * 6)
    assert r.counts() == d.fe.counts(1)[:3]


def test_refused_calls_change_nothing():
    """A repeated id, an id out of range, nsamp > nmax, Tcap too small and the r = 1 assertion row each return EINVAL; the next
    valid push gives exactly what it gives on a twin handle that never saw the bad call."""
    pcm = torch.from_numpy(noise(4, 8000, 10)).cuda()
    kw = dict(left=1, right=1, skip=2, max_chunk=3200, **FB["h40"])
    a, b = StreamingFrontEnd(4, **kw), StreamingFrontEnd(4, **kw)
    first = pcm[:, :3200].contiguous()
    fa, na = a.push(first)
    fb_, nb = b.push(first)
    assert na == nb and torch.equal(fa, fb_)
    nxt = pcm[:, 3200:6400].contiguous()
    bad = [dict(streams=[0, 1, 1, 3]), dict(streams=[0, 1, 2, 4]), dict(streams=[0, -1, 2, 3]), dict(samples=[3200, 3201, 1, 1]),
           dict(samples=[3200, -1, 1, 1]), dict(capacity=3),
           dict(samples=[3200, 3200, 100, 3200])]      # stream 2 holds 320 samples: 420 = one frame for a right context of one
    assert a.counts(2)[0] == 320
    for kwargs in bad:
        with pytest.raises(_capi.HipLibraryError, match=r"code -1"):
            a.push(nxt, **kwargs)
        for s in range(4):
            assert a.counts(s) == b.counts(s), kwargs
    with pytest.raises(_capi.HipLibraryError, match=r"code -1"):
        a.push(torch.zeros((4, 3202), dtype=torch.int16, device="cuda"))          # nmax > max_chunk
    with pytest.raises(_capi.HipLibraryError, match=r"code -1"):
        a.reset([0, 9])
    assert a.counts(0) == b.counts(0)
    fa, na = a.push(nxt)
    fb_, nb = b.push(nxt)
    assert na == nb and min(na) > 0 and torch.equal(fa.view(torch.int32), fb_.view(torch.int32))
    fa, na = a.push(pcm[:, 6400:].contiguous(), samples=[1600, 1, 0, 777], streams=[3, 2, 1, 0])
    fb_, nb = b.push(pcm[:, 6400:].contiguous(), samples=[1600, 1, 0, 777], streams=[3, 2, 1, 0])
    assert na == nb and torch.equal(fa.view(torch.int32), fb_.view(torch.int32))


def test_bit_identical_beside_an_mfma_tenant():
    """A context-and-skip schedule (80 bins, (2, 2), skip 3) beside the MDTC tenant on a second stream, as tests/test_hip_tenants.py
    does for the other kernels: bit-identical to the solo run."""
    from tests.test_hip_parity import build
    from wekws_amd import pack
    from wekws_amd.utils import synth
    cfg = dict(synth.MODEL_CONFIGS["mdtc_h64"])
    tm = build(cfg, synth.synth_state_dict(pack.model_spec(cfg), 99))
    tx = torch.from_numpy(synth.synth_feats(512, 98, cfg["input_dim"], seed=8)).cuda()
    streams = 384
    sizes = [4800, 161, 500, 399, 4800, 1, 2400]
    pcm = torch.from_numpy(noise(streams, sum(sizes), 11)).cuda()
    chunks, at = [], 0
    for k in sizes:
        chunks.append(pcm[:, at:at + k].contiguous())
        at += k

    def work():
        fe = StreamingFrontEnd(streams, left=2, right=2, skip=3, max_chunk=4800, **FB["p80"])
        return [fe.push(c, capacity=fe.max_frames(4800)) for c in chunks]

    solo = work()
    torch.cuda.synchronize()
    s_a, s_b = torch.cuda.Stream(), torch.cuda.Stream()
    for rnd in range(4):
        with torch.cuda.stream(s_b):
            for _ in range(8):
                tm(tx)
        with torch.cuda.stream(s_a):
            got = work()
        torch.cuda.synchronize()
        for k, ((g, ng), (r, nr)) in enumerate(zip(got, solo)):
            assert ng == nr and torch.equal(g.view(torch.int32), r.view(torch.int32)), (rnd, k)
