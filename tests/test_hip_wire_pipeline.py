"""GPU: wire encodings in front of the pipeline -- BatchedKeyWordSpotter / BatchedThresholdSpotter whose ``input_sample_rate`` holds
(rate, encoding) pairs, fed the bytes the streams arrive in -- against the same spotter over plain rates fed the host-decoded
int16 samples (tests/wire_ref.py) in the same calls: posteriors bit for bit, results equal.  The model and the settings are those
of tests/test_hip_resample_bank_pipeline.py."""
import numpy as np
import pytest
import torch

from tests import wire_ref as WR
from tests.test_hip_parity import build
from wekws_amd import pack
from wekws_amd.frontend import StreamingResamplerBank
from wekws_amd.stream import BatchedKeyWordSpotter, BatchedThresholdSpotter
from wekws_amd.utils import synth

pytestmark = pytest.mark.gpu


def wire_signal(rng, enc, n):
    if enc == "f32":
        return (rng.standard_normal(n) * 0.3).astype("<f4")
    if enc == "s16":
        return rng.integers(-12000, 12000, n).astype("<i2")
    return rng.integers(0, 256, n).astype(np.uint8)


def same_rows(a, b):
    assert [t is None for t in a] == [t is None for t in b]
    n = 0
    for x, y in zip(a, b):
        if x is not None:
            assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
            n += int(x.size(0))
    return n


def test_keyword_spotter_on_wire_bytes_equals_the_spotter_on_decoded_int16():
    name, fe_kw, kws = "fsmn_small", dict(num_bins=40, window="hamming", left=1, right=1, skip=2), {"k0": (1, 2), "k1": (7,)}
    cfg = dict(synth.MODEL_CONFIGS[name])
    model = build(cfg, synth.synth_state_dict(pack.model_spec(cfg), 5))
    spot = dict(min_frames=0, max_frames=40)
    members = [(8000, "mulaw"), 16000, (48000, "f32")]
    S = 6
    member = [(8000, "mulaw"), (8000, "mulaw"), (16000, "s16"), (16000, "s16"), (48000, "f32"), (48000, "f32")]
    # >= 3 frames at 16 kHz per chunk; odd sizes, so that rows end off a dword
    sizes = [[500, 1601, 803], [1600, 333, 1111], [1000, 3201, 1601], [3200, 999, 640], [3000, 9600, 4801], [7201, 3001, 2400]]
    rng = np.random.default_rng(12)
    sig = [wire_signal(rng, member[s][1], sum(sizes[s])) for s in range(S)]
    pcm = [WR.decode(member[s][1], sig[s]) for s in range(S)]
    wire = BatchedKeyWordSpotter(model, kws, 0.0, S, max_chunk=12000, input_sample_rate=members, **fe_kw, **spot)
    plain = BatchedKeyWordSpotter(model, kws, 0.0, S, max_chunk=12000, input_sample_rate=[8000, 16000, 48000], **fe_kw, **spot)
    assert isinstance(wire.resampler, StreamingResamplerBank) and wire.frontend.max_chunk == plain.frontend.max_chunk
    assert [wire.resampler.encoding_of(s) for s in range(S)] == ["mulaw"] * S        # streams start on the first member
    for s in range(S):
        wire.set_input_rate([s], 16000 if s == 2 else member[s])              # (a plain rate names its s16 member)
        plain.set_input_rate([s], member[s][0])
    assert [(wire.resampler.rate_of(s), wire.resampler.encoding_of(s)) for s in range(S)] == member
    with pytest.raises(ValueError, match="not in the bank"):
        wire.set_input_rate([0], (8000, "alaw"))
    pos = [0] * S
    frames = 0
    for k in range(3):
        ids = [4, 0, 2, 5, 1, 3]                                              # neighbouring rows differ in member
        cut = [slice(pos[s], pos[s] + sizes[s][k]) for s in ids]
        # bytes and arrays alike, each read in its stream's encoding
        chunks = [sig[s][c].tobytes() if b % 2 else sig[s][c].copy() for b, (s, c) in enumerate(zip(ids, cut))]
        out, probs, feats = wire.forward(chunks, streams=ids, return_probs=True)
        out1, probs1, feats1 = plain.forward([pcm[s][c].copy() for s, c in zip(ids, cut)], streams=ids, return_probs=True)
        frames += same_rows(probs, probs1)
        same_rows(feats, feats1)
        assert out == out1, k
        for s in ids:
            pos[s] += sizes[s][k]
            assert wire.resampler.counts(s) == plain.resampler.counts(s) and wire.resampler.counts(s)[0] == pos[s]
    assert frames > 40                                                        # (about 100: six streams of ~0.35 s at 50 frames/s)
    # one padded uint8 device tensor instead of the list: the same step
    wire.reset_all()
    plain.reset_all()
    ids = [1, 4, 2]
    raws = [sig[s][:sizes[s][0]] for s in ids]
    rows = [np.ascontiguousarray(r).view(np.uint8) for r in raws]
    host = np.zeros((3, (max(r.size for r in rows) + 3) // 4 * 4), dtype=np.uint8)
    for i, r in enumerate(rows):
        host[i, :r.size] = r
    out, probs, _ = wire.forward(torch.from_numpy(host).to("cuda"), streams=ids, samples=[r.size for r in raws], return_probs=True)
    out1, probs1, _ = plain.forward([pcm[s][:sizes[s][0]].copy() for s in ids], streams=ids, return_probs=True)
    assert same_rows(probs, probs1) > 0 and out == out1


def test_threshold_spotter_on_two_wire_members():
    cfg = dict(synth.MODEL_CONFIGS["mdtc_h64_80d"])
    model = build(cfg, synth.synth_state_dict(pack.model_spec(cfg), 5))
    names = ["hi_xiaowen", "nihao_wenwen"]
    fe_kw = dict(num_bins=80, window="povey", num_ceps=80, cepstral_lifter=22.0)
    S = 3
    member = [(8000, "alaw"), (48000, "f32"), (8000, "alaw")]
    sizes = [[800, 1201, 403], [4800, 7200, 2403], [1200, 799, 1600]]
    rng = np.random.default_rng(4)
    sig = [wire_signal(rng, member[s][1], sum(sizes[s])) for s in range(S)]
    pcm = [WR.decode(member[s][1], sig[s]) for s in range(S)]
    wire = BatchedThresholdSpotter(model, names, 0.0, S, max_chunk=7200, input_sample_rate=[(8000, "alaw"), (48000, "f32")],
                                   window_shift=5, **fe_kw)
    plain = BatchedThresholdSpotter(model, names, 0.0, S, max_chunk=7200, input_sample_rate=[8000, 48000], window_shift=5, **fe_kw)
    wire.set_input_rate([1], (48000, "f32"))
    plain.set_input_rate([1], 48000)
    pos = [0] * S
    rows, hit_any = 0, False
    for k in range(3):
        ids = [1, 0, 2]
        cut = [slice(pos[s], pos[s] + sizes[s][k]) for s in ids]
        out, probs, _ = wire.forward([sig[s][c].tobytes() for s, c in zip(ids, cut)], streams=ids, return_probs=True)
        out1, probs1, _ = plain.forward([pcm[s][c].copy() for s, c in zip(ids, cut)], streams=ids, return_probs=True)
        rows += same_rows(probs, probs1)
        assert out == out1, k
        hit_any |= any(bool(o) for o in out)
        for s in ids:
            pos[s] += sizes[s][k]
    assert rows > 30 and hit_any
