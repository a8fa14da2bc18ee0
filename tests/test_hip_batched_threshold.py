"""GPU: wekws_amd.stream.BatchedThresholdSpotter -- PCM chunks of several streams in, threshold detections out: the streaming
front end in MFCC mode, the model over its cache pool (KWSModel.forward_streams), the streaming threshold scan.

The model is synth.MODEL_CONFIGS["mdtc_h64_80d"], the reference's mdtc.yaml at its 80-d MFCC input (mdtc_small is declared at 40
inputs; the 80-d synthetic MDTC is the nearest configuration whose input_dim is the recipe's num_ceps).  The hits must be those of
ONE scan over the posteriors of the whole signal computed one-shot: model(Mfcc(...)(whole))[0]."""
import numpy as np
import pytest
import torch

from tests.helpers import TIGHT_K
from tests.test_hip_parity import build
from tests.test_hip_threshold_kws import whole_scan
from wekws_amd import pack
from wekws_amd.frontend import Mfcc
from wekws_amd.stream import BatchedThresholdSpotter
from wekws_amd.utils import synth

pytestmark = pytest.mark.gpu

STREAMS, NSAMP, WINDOW_SHIFT = 4, 24000, 5
NAMES = ["hi_xiaowen", "nihao_wenwen"]
FE = dict(num_bins=80, window="povey", num_ceps=80, cepstral_lifter=22.0, max_chunk=4000)


def signals():
    """(STREAMS, NSAMP) int16: noise under an envelope that changes every 800 samples, so that the posteriors move."""
    rng = np.random.default_rng(21)
    env = np.repeat(rng.uniform(50.0, 9000.0, size=(STREAMS, NSAMP // 800)), 800, axis=1)
    return np.clip(np.round(rng.standard_normal((STREAMS, NSAMP)) * env), -32767, 32767).astype(np.int16)


def plan_calls(rng):
    """Calls [(stream, samples)] until every stream is through: uneven chunks (some shorter than a frame), subsets, permuted."""
    todo = [NSAMP] * STREAMS
    calls = []
    while any(todo):
        live = [s for s in range(STREAMS) if todo[s]]
        pick = [s for s in live if rng.random() < 0.8] or live[:1]
        pick = [pick[i] for i in rng.permutation(len(pick))]
        call = []
        for s in pick:
            n = min(int(rng.choice([100, 399, 800, 801, 1600, 2399, 3200, 4000])), todo[s])
            todo[s] -= n
            call.append((s, n))
        calls.append(call)
    return calls


def separating_threshold(x):
    """A threshold in the upper part of the scores x with no score within 2 TIGHT_K of it: the middle of the widest gap between
    neighbouring scores from the 70 % to the 90 % quantile (a tenth of the scores at least lies above it)."""
    v = np.unique(np.asarray(x, np.float64))
    v = v[int(0.7 * len(v)):int(0.9 * len(v))]
    i = int(np.argmax(np.diff(v)))
    return 0.5 * (v[i] + v[i + 1])


def test_pcm_in_threshold_hits_out():
    cfg = dict(synth.MODEL_CONFIGS["mdtc_h64_80d"])
    assert cfg["input_dim"] == FE["num_ceps"] and cfg["output_dim"] == len(NAMES)
    sd = synth.synth_state_dict(pack.model_spec(cfg), 5)
    model = build(cfg, sd)
    pcm = signals()
    # one-shot: the whole signals through Mfcc and one forward
    whole = model(Mfcc(80, 80)(torch.from_numpy(pcm.astype(np.float32)).cuda()))[0].cpu().numpy()
    T = whole.shape[1]
    assert whole.shape == (STREAMS, 1 + (NSAMP - 400) // 160, 2) and np.isfinite(whole).all()
    th = [separating_threshold(whole[:, :, k]) for k in range(2)]
    for k in range(2):
        margin = float(np.abs(whole[:, :, k].astype(np.float64) - th[k]).min())
        print("keyword", k, "threshold", th[k], "nearest score at", margin)
        assert margin > 2 * TIGHT_K, (k, th[k], margin)           # rounding between the two paths cannot flip a decision
    want = [[whole_scan(whole[s, :, k], th[k], WINDOW_SHIFT) for k in range(2)] for s in range(STREAMS)]
    assert sum(len(w) for row in want for w in row) >= 8

    kws = BatchedThresholdSpotter(model, NAMES, th, STREAMS, window_shift=WINDOW_SHIFT, **FE)
    assert kws.frontend.feat_dim == 80
    pos = [0] * STREAMS
    got = [[[] for _ in range(2)] for _ in range(STREAMS)]
    probs_all = [[] for _ in range(STREAMS)]
    empty_rows = 0
    for call in plan_calls(np.random.default_rng(22)):
        ids = [s for s, _ in call]
        chunks = []
        for s, n in call:
            chunks.append(pcm[s, pos[s]:pos[s] + n].copy())
            pos[s] += n
        out, probs, _ = kws.forward(chunks, streams=ids, return_probs=True)
        for b, s in enumerate(ids):
            if probs[b] is None:
                assert out[b] == []
                empty_rows += 1
                continue
            probs_all[s].append(probs[b].cpu().numpy())
            for h in out[b]:
                got[s][NAMES.index(h["keyword"])].append((h["frame"], h["score"]))
                assert h["time"] == pytest.approx(h["frame"] * 0.01)
    assert pos == [NSAMP] * STREAMS and empty_rows > 0
    worst = 0.0
    for s in range(STREAMS):
        stream_probs = np.concatenate(probs_all[s])
        assert stream_probs.shape == (T, 2)
        worst = max(worst, float(np.abs(stream_probs.astype(np.float64) - whole[s]).max()))
        for k in range(2):
            assert [a for a, _ in got[s][k]] == want[s][k], (s, k)
            assert all(abs(v - float(whole[s, a, k])) <= TIGHT_K for a, v in got[s][k]), (s, k)
    print("streamed vs one-shot posteriors: max |diff| =", worst)
    assert worst <= TIGHT_K, worst
    # reset_all: a stream starts over -- front end, cache and detector
    kws.reset_all([2])
    assert kws.frontend.counts(2) == (0, -1, 0, 0) and kws.spotter.best(2) == ([-np.inf] * 2, [-1] * 2)
    out = kws.forward([pcm[2, :4000].copy()], streams=[2])
    n0 = 1 + (4000 - 400) // 160                                  # (the model is causal: its first frames are the one-shot's)
    first = sorted((a, NAMES[k]) for k in range(2) for a in whole_scan(whole[2, :n0, k], th[k], WINDOW_SHIFT))
    assert [(h["frame"], h["keyword"]) for h in out[0]] == first


def test_a_model_without_a_per_frame_keyword_head_is_refused():
    cfg = dict(synth.MODEL_CONFIGS["mdtc_h64_80d"])
    model = build(cfg, synth.synth_state_dict(pack.model_spec(cfg), 5))
    with pytest.raises(ValueError):
        BatchedThresholdSpotter(model, ["only_one"], 0.5, STREAMS, **FE)
    pooled = dict(synth.MODEL_CONFIGS["mdtc_small_global12"])
    pm = build(pooled, synth.synth_state_dict(pack.model_spec(pooled), 5))
    with pytest.raises(ValueError):
        BatchedThresholdSpotter(pm, [f"k{i}" for i in range(12)], 0.5, STREAMS, num_bins=40)
    with pytest.raises(TypeError):
        BatchedThresholdSpotter(model, NAMES, 0.5, STREAMS, min_frames=3, **FE)
