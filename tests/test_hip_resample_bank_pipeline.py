"""GPU: the rate bank in front of the pipeline -- BatchedKeyWordSpotter / BatchedThresholdSpotter with a sequence of rates in
``input_sample_rate`` -- against spotters built for ONE rate each (and none), stream by stream: the features the model is given
bit for bit, the result dicts equal."""
import numpy as np
import pytest
import torch

from tests.test_hip_parity import build
from wekws_amd import _capi, pack
from wekws_amd.frontend import Resample, StreamingResampler, StreamingResamplerBank
from wekws_amd.stream import BatchedKeyWordSpotter, BatchedThresholdSpotter
from wekws_amd.utils import synth

pytestmark = pytest.mark.gpu


def test_spotter_of_mixed_rates_equals_the_single_rate_spotters_stream_by_stream():
    name, fe_kw, kws = "fsmn_small", dict(num_bins=40, window="hamming", left=1, right=1, skip=2), {"k0": (1, 2), "k1": (7,)}
    cfg = dict(synth.MODEL_CONFIGS[name])
    model = build(cfg, synth.synth_state_dict(pack.model_spec(cfg), 5))
    S = 4
    rate = [48000, 48000, 16000, 8000]
    rng = np.random.default_rng(9)
    # per stream; >= 3 frames at 16 kHz per chunk (the 48 kHz sizes of the single-rate test, a third and a sixth of them)
    sizes = [[3000, 9600, 4801], [7200, 3001, 7200], [1000, 3200, 1601], [2000, 900, 0]]
    sig = rng.integers(-12000, 12000, (S, max(sum(s) for s in sizes)), dtype=np.int16)
    spot = dict(min_frames=0, max_frames=40)
    mixed = BatchedKeyWordSpotter(model, kws, 0.0, S, max_chunk=12000, input_sample_rate=[16000, 48000, 8000], **fe_kw, **spot)
    assert isinstance(mixed.resampler, StreamingResamplerBank) and mixed.resampler.out_dtype == torch.int16
    assert mixed.resampler.max_chunk == 12000 and mixed.frontend.max_chunk == mixed.resampler.max_out(12000) >= 24000
    assert [mixed.resampler.rate_of(s) for s in range(S)] == [16000] * S          # streams start at the first rate
    mixed.set_input_rate([0, 1], 48000)
    mixed.set_input_rate([3], 8000)
    assert [mixed.resampler.rate_of(s) for s in range(S)] == rate
    with pytest.raises(ValueError, match="not in the bank"):
        mixed.set_input_rate([2], 44100)
    alone = {48000: BatchedKeyWordSpotter(model, kws, 0.0, S, max_chunk=12000, input_sample_rate=48000, **fe_kw, **spot),
             16000: BatchedKeyWordSpotter(model, kws, 0.0, S, max_chunk=12000, **fe_kw, **spot),
             8000: BatchedKeyWordSpotter(model, kws, 0.0, S, max_chunk=12000, input_sample_rate=8000, **fe_kw, **spot)}
    assert alone[16000].resampler is None and type(alone[48000].resampler) is StreamingResampler
    with pytest.raises(ValueError, match="sequence of rates"):
        alone[48000].set_input_rate([0], 48000)
    pos = [0] * S
    rows, hits = ({k: [[] for _ in range(S)] for k in ("mixed", "alone")} for _ in range(2))
    for k in range(3):
        ids = [s for s in (2, 0, 3, 1) if sizes[s][k] > 0]                       # neighbouring rows differ in rate
        chunks = [sig[s, pos[s]:pos[s] + sizes[s][k]].copy() for s in ids]
        out, _, x = mixed.forward(chunks, streams=ids, return_probs=True)
        for r in sorted(set(rate)):
            part = [b for b, s in enumerate(ids) if rate[s] == r]
            if not part:
                continue
            out1, _, x1 = alone[r].forward([chunks[b] for b in part], streams=[ids[b] for b in part], return_probs=True)
            for b, o, f in zip(part, out1, x1):
                rows["alone"][ids[b]].append(f)
                hits["alone"][ids[b]].append(o)
        for b, s in enumerate(ids):
            pos[s] += sizes[s][k]
            assert mixed.resampler.counts(s)[0] == pos[s]
            rows["mixed"][s].append(x[b])
            hits["mixed"][s].append(out[b])
    fired = 0
    for s in range(S):
        assert [f is None for f in rows["mixed"][s]] == [f is None for f in rows["alone"][s]], s
        a = torch.cat([f for f in rows["mixed"][s] if f is not None])
        b = torch.cat([f for f in rows["alone"][s] if f is not None])
        assert a.shape == b.shape and a.size(0) > 5 and torch.equal(a.view(torch.int32), b.view(torch.int32)), (s, rate[s])
        assert hits["mixed"][s] == hits["alone"][s], (s, rate[s])
        fired += any(bool(h) for h in hits["mixed"][s])
    assert fired >= 1
    # set_input_rate on a running stream restarts it: the resampler, the front end, and (with them) the session
    assert mixed.resampler.counts(1)[0] == pos[1] and mixed.frontend.counts(1) != (0, -1, 0, 0)
    mixed.set_input_rate([1], 8000)
    assert mixed.resampler.rate_of(1) == 8000 and mixed.resampler.counts(1) == (0, 0, 0, 0) and mixed.frontend.counts(1) == (0, -1, 0, 0)
    assert mixed.resampler.counts(0)[0] == pos[0] and mixed.frontend.counts(0) != (0, -1, 0, 0)
    alone[8000].reset_all([1])
    chunk = [sig[1, :2000].copy()]
    assert mixed.forward(chunk, streams=[1]) == alone[8000].forward(chunk, streams=[1])
    assert mixed.resampler.counts(1)[0] == 2000
    # a refused change restarts nothing
    before = (mixed.resampler.counts(0), mixed.frontend.counts(0))
    with pytest.raises(_capi.HipLibraryError, match="outside"):
        mixed.set_input_rate([0, S], 16000)
    assert (mixed.resampler.counts(0), mixed.frontend.counts(0)) == before and mixed.resampler.rate_of(0) == 48000


def test_threshold_spotter_with_two_rates():
    """Streams at 16 kHz and 48 kHz in one BatchedThresholdSpotter against a spotter WITHOUT a resampler that is given, row for
    row, the samples the one-shot kernel makes of each stream's whole signal -- the same rows in the same calls, so the model
    and the detector see the same batch."""
    cfg = dict(synth.MODEL_CONFIGS["mdtc_h64_80d"])
    model = build(cfg, synth.synth_state_dict(pack.model_spec(cfg), 5))
    names = ["hi_xiaowen", "nihao_wenwen"]
    fe_kw = dict(num_bins=80, window="povey", num_ceps=80, cepstral_lifter=22.0)
    S = 3
    rate = [16000, 48000, 48000]
    sizes = [[1600, 2400, 801], [4800, 7200, 2403], [7200, 4800, 2400]]
    rng = np.random.default_rng(4)
    sig = rng.integers(-12000, 12000, (S, 14403), dtype=np.int16)
    mixed = BatchedThresholdSpotter(model, names, 0.0, S, max_chunk=7200, input_sample_rate=(16000, 48000), window_shift=5, **fe_kw)
    assert isinstance(mixed.resampler, StreamingResamplerBank) and mixed.frontend.max_chunk == mixed.resampler.max_out(7200)
    mixed.set_input_rate([1, 2], 48000)
    at16 = BatchedThresholdSpotter(model, names, 0.0, S, max_chunk=7300, window_shift=5, **fe_kw)
    whole = [sig[0]] + [Resample(48000, 16000, out_dtype=torch.int16)(torch.from_numpy(sig[s:s + 1]).to("cuda"))[0].cpu().numpy()
                        for s in (1, 2)]
    pos = [0] * S
    hit_any, rows = False, 0
    for k in range(3):
        ids = [1, 0, 2]
        chunks = [sig[s, pos[s]:pos[s] + sizes[s][k]].copy() for s in ids]
        before = [mixed.resampler.counts(s)[1] for s in ids]
        out, _, x = mixed.forward(chunks, streams=ids, return_probs=True)
        after = [mixed.resampler.counts(s)[1] for s in ids]
        out1, _, x1 = at16.forward([whole[s][a:b].copy() for s, a, b in zip(ids, before, after)], streams=ids, return_probs=True)
        for b, s in enumerate(ids):
            pos[s] += sizes[s][k]
            assert mixed.resampler.counts(s)[0] == pos[s] and mixed.resampler.rate_of(s) == rate[s]
            assert (x[b] is None) == (x1[b] is None)
            if x[b] is not None:
                assert torch.equal(x[b].view(torch.int32), x1[b].view(torch.int32)), (k, s)
                rows += int(x[b].size(0))
            assert out[b] == out1[b], (k, s)
            hit_any |= bool(out[b])
    assert hit_any and rows > 30
