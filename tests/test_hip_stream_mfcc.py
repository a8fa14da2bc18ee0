"""GPU: the MFCC mode of the streaming front end (StreamingFrontEnd(num_ceps=...) over wekws_hip_stream_frontend_create_mfcc).

The wave that finished a frame applies the DCT and the lifter with the chain and the matrix of the one-shot kernel, so every row a
stream delivers is a GATHER from ``dct_lifter(Fbank(...)(whole signal), num_ceps, lifter)`` -- bit for bit, as the log-mel mode is a
gather from ``Fbank(...)(whole signal)`` (tests/test_hip_stream_frontend.py, whose driver and schedules run here)."""
import numpy as np
import pytest
import torch

from oracle import kaldi_feats_oracle as kf, splice_oracle
from tests import stream_frontend_ref as sref
from tests import test_hip_stream_frontend as sf
from tests.helpers import K_DCT
from wekws_amd import _capi
from wekws_amd.frontend import Fbank, StreamingFrontEnd, dct_lifter

pytestmark = pytest.mark.gpu

P128 = dict(num_bins=128, window="povey", sample_rate=8000, frame_length=400, frame_shift=160)     # the most bins the library takes
MF = {  # name -> (fbank settings, cepstra, lifter)
    "p80": (sf.FB["p80"], 80, 22.0),           # the recipe: two cepstra per lane
    "h40": (sf.FB["h40"], 13, 22.0),           # fewer cepstra than bins, fewer than a wave
    "h16_8k": (sf.FB["h16_8k"], 16, 22.0),
    "h40_q0": (sf.FB["h40"], 13, 0.0),         # no lifter
    "p128": (P128, 128, 22.0),                 # num_bins = num_ceps = 128: the limit
}
_cache = {}


def settings(name):
    fb, nc, q = MF[name]
    return dict(fb, num_ceps=nc, cepstral_lifter=q)


def one_shot(name, pcm, key=None):
    """(log-mel (streams, T, bins), MFCC (streams, T, cepstra)) of the whole signals by the one-shot kernels; once per key."""
    if key is not None and (name, key) in _cache:
        return _cache[(name, key)]
    fb, nc, q = MF[name]
    logmel = Fbank(fb["num_bins"], fb.get("sample_rate", 16000), fb.get("frame_length"), fb.get("frame_shift"), fb["window"])(
        torch.from_numpy(pcm).cuda())
    out = logmel.cpu().numpy(), dct_lifter(logmel, nc, q).cpu().numpy()
    if key is not None:
        _cache[(name, key)] = out
    return out


class Driver(sf.Driver):
    """tests/test_hip_stream_frontend.py's driver over a front end in MFCC mode: `feats` are the one-shot cepstra."""

    def __init__(self, name, pcm, left=0, right=0, skip=1, max_chunk=4800, feats=None):
        fb = MF[name][0]
        self.L, self.S = fb.get("frame_length", 400), fb.get("frame_shift", 160)
        self.pcm = pcm
        self.n = pcm.shape[0]
        self.fe = StreamingFrontEnd(self.n, left=left, right=right, skip=skip, max_chunk=max_chunk, **settings(name))
        self.refs = [sref.StreamRef(self.L, self.S, left, right, skip) for _ in range(self.n)]
        self.pos = [0] * self.n
        self.feats = feats
        self.rows = [[] for _ in range(self.n)]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("ctx", [(0, 0, 1), (2, 2, 3), (1, 1, 2)], ids=lambda c: "ctx%d%d_skip%d" % c)
@pytest.mark.parametrize("name", sorted(MF))
def test_rows_equal_the_one_shot_mfcc(name, ctx):
    """5 streams of 12,000 samples in the seeded schedule of the log-mel test (chunks of 0 / 1 / 2 / 159 .. 401 / 4800 / random:
    odd leftovers, chunks shorter than a frame, held rows; calls over subsets of the streams in permuted order): every call's rows
    are the restatement's gather from the one-shot cepstra, bit for bit.  Without context the concatenation is the one-shot MFCC
    itself; with context, big chunks concatenate to splice_skip(one-shot MFCC)."""
    left, right, skip = ctx
    nc = MF[name][1]
    pcm = sf.noise(5, 12000, 1)
    _, feats = one_shot(name, pcm, "t1")
    rng = np.random.default_rng(2 + 10 * left + skip)
    d = Driver(name, pcm, left, right, skip, feats=feats)
    assert d.fe.feat_dim == nc * (left + right + 1)
    scheds = [sf.schedule(rng, 12000) for _ in range(5)]
    assert any(n % 2 for s in scheds for n in s) and any(n < d.L for s in scheds for n in s)
    assert d.run(rng, scheds) > 5                                       # (every call checked row by row in Driver.call)
    if ctx == (0, 0, 1):
        for s in range(5):
            got = d.delivered(s)
            assert got.shape == (1 + (12000 - d.L) // d.S, nc)          # every frame of the signal, once
            assert np.array_equal(bits(got), bits(feats[s])), s
        return
    d2 = Driver(name, pcm, left, right, skip, feats=feats)
    lo = d2.S * (2 * right + 3)
    d2.run(rng, [sf.schedule(rng, 12000, big=True, lo=lo) for _ in range(5)])
    want = splice_oracle.splice_skip(feats, left, right, skip)
    for s in range(5):
        got = d2.delivered(s)
        assert got.shape[0] >= want.shape[1] - (lo // d2.S + 2 * right) // skip - 1
        assert np.array_equal(bits(got), bits(want[s, :got.shape[0]])), s


def test_streamed_rows_against_float64():
    """The recipe's rows against the float64 DCT / lifter of the log-mel rows they were made from, in the unit of
    oracle/kaldi_feats_oracle.py::dct_lifter_scale, at the bar of the one-shot kernel (tests/test_hip_mfcc_f64.py)."""
    pcm = sf.noise(5, 12000, 1)
    logmel, feats = one_shot("p80", pcm, "t1")
    rng = np.random.default_rng(7)
    d = Driver("p80", pcm, feats=feats)
    d.run(rng, [sf.schedule(rng, 12000) for _ in range(5)])
    for s in range(5):
        got = d.delivered(s).astype(np.float64)
        assert got.shape == feats[s].shape and np.isfinite(got).all()
        u = float((np.abs(got - kf.dct_lifter(logmel[s], 80, 22.0, dtype=np.float64)) / kf.dct_lifter_scale(logmel[s], 80, 22.0)).max())
        print("stream", s, "u =", u)
        assert u <= K_DCT, (s, u)


def test_reset_restarts_the_streams_it_names():
    """After reset the named streams get the first-chunk replicate pad again -- `left` copies of the first new frame, each of
    cepstral width -- and phase 0; the others go on."""
    name, nc = "h40", 13
    pcm = sf.noise(6, 12000, 9)
    _, feats = one_shot(name, pcm, "t5")
    d = Driver(name, pcm, 2, 2, 3, feats=feats)
    ids = list(range(6))
    d.call(ids, [4800] * 6)
    d.call(ids, [1001] * 6)
    assert d.fe.counts(2)[:3] == (361, 4, 1)
    before = [d.fe.counts(s) for s in ids]
    d.fe.reset([1, 4])
    for s in ids:
        assert d.fe.counts(s) == ((0, -1, 0, 0) if s in (1, 4) else before[s])
    pcm2 = pcm.copy()
    for s in (1, 4):
        pcm2[s, :12000 - 5801] = pcm[s, 5801:]
        d.refs[s].reset()
        d.pos[s] = 0
    d.pcm = pcm2
    feats2 = feats.copy()
    fresh = one_shot(name, pcm2[[1, 4]])[1]
    feats2[1], feats2[4] = fresh[0], fresh[1]
    d.feats = feats2
    out, frames = d.call(ids, [3000] * 6)          # checked row by row
    assert out.shape[2] == 5 * nc
    assert frames[1] == frames[4] and frames[1] != frames[0]
    assert np.array_equal(out[1, 0, :nc], out[1, 0, nc:2 * nc]) and np.array_equal(out[1, 0, :nc], out[1, 0, 2 * nc:3 * nc])
    assert np.array_equal(bits(out[1, 0, :nc]), bits(fresh[0][0]))
    d.call(ids, [1500] * 6)
    assert d.refs[1].counts() == d.fe.counts(1)[:3]


def test_refused_calls_change_nothing():
    """The refusals of the log-mel test on an MFCC handle: each returns EINVAL, and the next valid push gives exactly what it
    gives on a twin handle that never saw the bad call."""
    pcm = torch.from_numpy(sf.noise(4, 8000, 10)).cuda()
    kw = dict(left=1, right=1, skip=2, max_chunk=3200, **settings("h40"))
    a, b = StreamingFrontEnd(4, **kw), StreamingFrontEnd(4, **kw)
    first = pcm[:, :3200].contiguous()
    fa, na = a.push(first)
    fb_, nb = b.push(first)
    assert na == nb and fa.shape[2] == 39 and torch.equal(fa.view(torch.int32), fb_.view(torch.int32))
    nxt = pcm[:, 3200:6400].contiguous()
    bad = [dict(streams=[0, 1, 1, 3]), dict(streams=[0, 1, 2, 4]), dict(streams=[0, -1, 2, 3]), dict(samples=[3200, 3201, 1, 1]),
           dict(samples=[3200, -1, 1, 1]), dict(capacity=3), dict(samples=[3200, 3200, 100, 3200])]
    assert a.counts(2)[0] == 320
    for kwargs in bad:
        with pytest.raises(_capi.HipLibraryError, match=r"code -1"):
            a.push(nxt, **kwargs)
        for s in range(4):
            assert a.counts(s) == b.counts(s), kwargs
    with pytest.raises(_capi.HipLibraryError, match=r"code -1"):
        a.push(torch.zeros((4, 3202), dtype=torch.int16, device="cuda"))          # nmax > max_chunk
    with pytest.raises(ValueError):
        a.push(nxt, out=torch.zeros((4, a.max_frames(3200), 120), device="cuda"))  # a log-mel-wide buffer
    fa, na = a.push(nxt)
    fb_, nb = b.push(nxt)
    assert na == nb and min(na) > 0 and torch.equal(fa.view(torch.int32), fb_.view(torch.int32))
    fa, na = a.push(pcm[:, 6400:].contiguous(), samples=[1600, 1, 0, 777], streams=[3, 2, 1, 0])
    fb_, nb = b.push(pcm[:, 6400:].contiguous(), samples=[1600, 1, 0, 777], streams=[3, 2, 1, 0])
    assert na == nb and torch.equal(fa.view(torch.int32), fb_.view(torch.int32))


def test_bit_identical_beside_an_mfma_tenant():
    """The recipe's front end with context and skip beside the MDTC tenant on a second stream: bit-identical to the solo run (the
    DCT epilogue is vector arithmetic next to possible MFMA waves: wekws_amd/csrc/pk_safe.hip.h)."""
    from tests.test_hip_parity import build
    from wekws_amd import pack
    from wekws_amd.utils import synth
    cfg = dict(synth.MODEL_CONFIGS["mdtc_h64"])
    tm = build(cfg, synth.synth_state_dict(pack.model_spec(cfg), 99))
    tx = torch.from_numpy(synth.synth_feats(512, 98, cfg["input_dim"], seed=8)).cuda()
    streams = 384
    sizes = [4800, 161, 500, 399, 4800, 1, 2400]
    pcm = torch.from_numpy(sf.noise(streams, sum(sizes), 11)).cuda()
    chunks, at = [], 0
    for k in sizes:
        chunks.append(pcm[:, at:at + k].contiguous())
        at += k

    def work():
        fe = StreamingFrontEnd(streams, left=2, right=2, skip=3, max_chunk=4800, **settings("p80"))
        return [fe.push(c, capacity=fe.max_frames(4800)) for c in chunks]

    solo = work()
    torch.cuda.synchronize()
    assert solo[0][0].shape[2] == 400 and solo[0][0].any()
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


def test_log_mel_handle_beside_an_mfcc_handle():
    """Both modes in one process: a log-mel handle created after an MFCC one, and pushed to in turns with it, still returns the
    one-shot log-mel bits, and the MFCC handle the one-shot cepstra."""
    pcm = sf.noise(3, 8000, 12)
    logmel, ceps = one_shot("p80", pcm)
    mf = StreamingFrontEnd(3, max_chunk=4000, **settings("p80"))
    fb = StreamingFrontEnd(3, max_chunk=4000, **sf.FB["p80"])
    assert (mf.feat_dim, fb.feat_dim) == (80, 80) and mf.num_ceps == 80 and fb.num_ceps is None
    rows = {"mf": [], "fb": []}
    for at, n in ((0, 4000), (4000, 1601), (5601, 2399)):
        chunk = torch.from_numpy(pcm[:, at:at + n].copy()).cuda()
        for key, fe in (("mf", mf), ("fb", fb)):
            f, k = fe.push(chunk)
            assert len(set(k)) == 1
            rows[key].append(f[:, :k[0]].cpu().numpy())
    got_mf, got_fb = np.concatenate(rows["mf"], 1), np.concatenate(rows["fb"], 1)
    assert got_fb.shape == logmel.shape and np.array_equal(bits(got_fb), bits(logmel))
    assert got_mf.shape == ceps.shape and np.array_equal(bits(got_mf), bits(ceps))
    assert not np.array_equal(got_mf, got_fb)
