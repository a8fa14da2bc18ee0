"""GPU: wekws_amd.stream.BatchedKeyWordSpotter -- PCM chunks of several streams in, KeyWordSpotter.forward's result per
stream out: the streaming front end, the model with its carried cache (rows grouped by frame count), the CTC decoder."""
import numpy as np
import pytest
import torch

from oracle import kws_oracle
from tests import ctc_kws_ref as R
from tests.test_hip_parity import build
from wekws_amd import pack
from wekws_amd.frontend import StreamingFrontEnd
from wekws_amd.stream import BatchedKeyWordSpotter
from wekws_amd.utils import synth

pytestmark = pytest.mark.gpu

CASES = {  # model -> (front-end settings, keywords)
    "ds_tcn_h64_ctc20": (dict(num_bins=40, window="hamming"), {"k0": (3, 4), "k1": (5,)}),
    "fsmn_small": (dict(num_bins=40, window="hamming", left=1, right=1, skip=2), {"k0": (1, 2), "k1": (7,)}),
    "gru_1x128": (dict(num_bins=40, window="povey"), {"k0": (1,)}),          # cache batch axis 1
}
STREAMS, CALLS = 6, 7


def plan_calls(rng):
    """Per call: [(stream, chunk size)] -- streams start at different calls, uneven chunks, some left out, permuted."""
    calls = []
    for c in range(CALLS):
        live = [s for s in range(STREAMS) if s // 2 <= c]
        pick = [s for s in live if rng.random() < 0.8] or live[:1]
        pick = [pick[i] for i in rng.permutation(len(pick))]
        # (>= 800 samples: at least three frames, the right context of one never trips the reference's assertion)
        calls.append([(s, int(rng.choice([800, 801, 1600, 2399, 3200, 4000]))) for s in pick])
    return calls


@pytest.mark.parametrize("name", sorted(CASES))
def test_pcm_in_detection_out(name):
    fe_kw, kws = CASES[name]
    cfg = dict(synth.MODEL_CONFIGS[name])
    sd = synth.synth_state_dict(pack.model_spec(cfg), 5)
    model = build(cfg, sd)
    rng = np.random.default_rng(3)
    calls = plan_calls(rng)
    pcm = rng.integers(-12000, 12000, size=(STREAMS, sum(n for c in calls for _, n in c)), dtype=np.int16)
    skip = fe_kw.get("skip", 1)
    spot = dict(min_frames=0, max_frames=40)
    together = BatchedKeyWordSpotter(model, kws, 0.0, STREAMS, max_chunk=4000, **fe_kw, **spot)
    alone = BatchedKeyWordSpotter(model, kws, 0.0, STREAMS, max_chunk=4000, **fe_kw, **spot)
    twin = StreamingFrontEnd(STREAMS, max_chunk=4000, **fe_kw)
    orc = [R.Spotter(list(kws.values()), 0.0, min_frames=0, max_frames=40, downsampling=skip) for _ in range(STREAMS)]
    ocache = [None] * STREAMS
    pos = [0] * STREAMS
    seen_counts, fired = set(), 0
    for call in calls:
        ids = [s for s, _ in call]
        chunks = []
        for s, n in call:
            chunks.append(pcm[s, pos[s]:pos[s] + n].copy())
            pos[s] += n
        out, probs, xs = together.forward(chunks, streams=ids, return_probs=True)
        feats, frames = twin.push(chunks, streams=ids)
        seen_counts.add(len({f for f in frames if f > 0}))
        for b, s in enumerate(ids):
            if frames[b] <= 0:
                assert out[b] == {} and probs[b] is None
                continue
            # the model was given the front end's own rows
            assert torch.equal(xs[b].view(torch.int32), feats[b, :frames[b]].view(torch.int32)), (s, frames[b])
            # posteriors: the oracle on the same features with ITS carried cache
            want, ocache[s] = kws_oracle.forward(cfg, sd, xs[b].cpu().numpy()[None], ocache[s], softmax=True)
            got = probs[b].cpu().numpy()
            assert float(np.abs(got - want[0]).max()) <= 1e-4, (name, s, float(np.abs(got - want[0]).max()))
            # detection: the host restatement on the returned device posteriors, exactly
            assert out[b] == R.as_result_dict(orc[s].step(got), list(kws)), (name, s)
            fired += int(out[b].get("state", 0) == 1)
        # rows of different frame counts in one call == each stream pushed alone
        for b, s in enumerate(ids):
            assert alone.forward([chunks[b]], streams=[s]) == [out[b]], (name, s)
    assert max(seen_counts) >= 2                    # some call held rows of different frame counts
    # reset_all: the stream starts over -- front end, cache and decoder
    together.reset_all([1])
    assert together.frontend.counts(1) == (0, -1, 0, 0)
    axis = together.cache_axis
    assert not together.cache.select(axis, 1).any() and together.cache.select(axis, 0).any()
    again = BatchedKeyWordSpotter(model, kws, 0.0, STREAMS, max_chunk=4000, **fe_kw, **spot)
    chunk = [pcm[1, :3200].copy()]
    assert together.forward(chunk, streams=[1]) == again.forward(chunk, streams=[1])
