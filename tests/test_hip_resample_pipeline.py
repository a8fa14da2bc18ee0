"""GPU: the resampler in front of the pipeline -- BatchedKeyWordSpotter(input_sample_rate=48000) and kws_main on a 48 kHz wav --
against the same pipeline at 16 kHz fed the one-shot resampled signal; kws_main on a 16 kHz wav against its recorded output."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.test_hip_parity import build
from tests.test_runtime_cpp import KWS_MAIN, build_runtime, write_wav
from wekws_amd import pack
from wekws_amd.frontend import Fbank, Resample
from wekws_amd.stream import BatchedKeyWordSpotter
from wekws_amd.utils import synth

pytestmark = pytest.mark.gpu


def test_spotter_at_48k_equals_the_16k_spotter_on_the_resampled_signal():
    name, fe_kw, kws = "fsmn_small", dict(num_bins=40, window="hamming", left=1, right=1, skip=2), {"k0": (1, 2), "k1": (7,)}
    cfg = dict(synth.MODEL_CONFIGS[name])
    model = build(cfg, synth.synth_state_dict(pack.model_spec(cfg), 5))
    S = 3
    rng = np.random.default_rng(9)
    sizes = [[3000, 9600, 4801], [7200, 3001, 7200], [12000, 5400, 0]]          # per stream; >= 3 frames at 16 kHz per chunk
    sig = rng.integers(-12000, 12000, (S, max(sum(s) for s in sizes)), dtype=np.int16)
    spot = dict(min_frames=0, max_frames=40)
    at48 = BatchedKeyWordSpotter(model, kws, 0.0, S, max_chunk=12000, input_sample_rate=48000, **fe_kw, **spot)
    at16 = BatchedKeyWordSpotter(model, kws, 0.0, S, max_chunk=4100, **fe_kw, **spot)
    assert at16.resampler is None and at48.resampler.out_dtype == torch.int16 and at48.resampler.max_chunk == 12000
    whole = Resample(48000, 16000, out_dtype=torch.int16)(torch.from_numpy(sig).to("cuda")).cpu().numpy()
    pos = [0] * S
    rows48, rows16 = [[] for _ in range(S)], [[] for _ in range(S)]
    hits48, hits16 = [[] for _ in range(S)], [[] for _ in range(S)]
    for k in range(3):
        ids = [s for s in (2, 0, 1) if sizes[s][k] > 0]
        chunks = [sig[s, pos[s]:pos[s] + sizes[s][k]].copy() for s in ids]
        before = [at48.resampler.counts(s)[1] for s in ids]
        out48, _, x48 = at48.forward(chunks, streams=ids, return_probs=True)
        after = [at48.resampler.counts(s)[1] for s in ids]
        out16, _, x16 = at16.forward([whole[s, a:b].copy() for s, a, b in zip(ids, before, after)], streams=ids, return_probs=True)
        for b, s in enumerate(ids):
            pos[s] += sizes[s][k]
            assert at48.resampler.counts(s)[0] == pos[s]
            if x48[b] is not None:
                rows48[s].append(x48[b])
            if x16[b] is not None:
                rows16[s].append(x16[b])
            hits48[s].append(out48[b])
            hits16[s].append(out16[b])
    for s in range(S):
        a, b = torch.cat(rows48[s]), torch.cat(rows16[s])
        assert a.shape == b.shape and a.size(0) > 10 and torch.equal(a.view(torch.int32), b.view(torch.int32)), s
        assert hits48[s] == hits16[s] and any(h for h in hits48[s]), s
    # reset_all also returns the resampler's streams to empty
    at48.reset_all([1])
    assert at48.resampler.counts(1) == (0, 0, 0, 0) and at48.resampler.counts(0)[0] == pos[0]
    assert at48.frontend.counts(1) == (0, -1, 0, 0)


def test_kws_main_resamples_a_48k_wav(tmp_path):
    build_runtime()
    name, chunk = "ds_tcn_h64", 80
    cfg = dict(synth.MODEL_CONFIGS[name])
    sd = synth.synth_state_dict(pack.model_spec(cfg), 1234)
    desc, blob = pack.pack(cfg, sd)
    model_path = str(tmp_path / "model.wekwship")
    pack.save_packed(model_path, desc, blob)
    pcm = (synth.synth_pcm(1, 60000, seed=11, kind="noise")[0] * 0.5 + synth.synth_pcm(1, 60000, kind="sine")[0])
    pcm = np.clip(np.round(pcm), -32768, 32767).astype(np.int16)
    wav = str(tmp_path / "t48.wav")
    write_wav(wav, pcm, rate=48000)
    r = subprocess.run([KWS_MAIN, "40", str(chunk), model_path, wav], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [line.split() for line in r.stdout.strip().splitlines()]
    assert all(w[0] == "frame" and w[2] == "prob" for w in rows) and [int(w[1]) for w in rows] == list(range(len(rows)))
    got = np.array([[float(v) for v in w[3:]] for w in rows], np.float32)
    # Resample -> Fbank -> the model, chunk by chunk with the carried cache, in Python
    x = torch.from_numpy(pcm.astype(np.float32))[None].to("cuda")
    feats = Fbank(num_bins=40)(Resample(48000)(x))
    assert feats.size(1) == 1 + (20000 - 400) // 160
    m = build(cfg, sd)
    cache, ys = None, []
    for t in range(0, feats.size(1), chunk):
        y, cache = m(feats[:, t:t + chunk].contiguous(), cache)
        ys.append(y)
    want = torch.cat(ys, 1)[0].cpu().numpy()
    assert got.shape == want.shape
    assert float(np.abs(got - want).max()) <= 1e-4


def test_kws_main_on_a_16k_wav_prints_what_it_printed_before_the_resampler(tmp_path):
    """A 16 kHz file takes exactly the path it took before kws_main learnt to resample: its output for this deterministic model
    and wav is byte-identical to the text recorded from the commit before the resampler (tests/golden/kws_main_16k_ds_tcn_h64.txt,
    `kws_main 40 80` on seed-1234 ds_tcn_h64 and the wav below), and its posteriors are those of Fbank -> the model in Python,
    no resampler anywhere."""
    build_runtime()
    name, chunk = "ds_tcn_h64", 80
    cfg = dict(synth.MODEL_CONFIGS[name])
    sd = synth.synth_state_dict(pack.model_spec(cfg), 1234)
    desc, blob = pack.pack(cfg, sd)
    model_path = str(tmp_path / "model.wekwship")
    pack.save_packed(model_path, desc, blob)
    pcm = (synth.synth_pcm(1, 40000, seed=11, kind="noise")[0] * 0.5 + synth.synth_pcm(1, 40000, kind="sine")[0])
    pcm = np.clip(np.round(pcm), -32768, 32767).astype(np.int16)
    wav = str(tmp_path / "t16.wav")
    write_wav(wav, pcm)
    r = subprocess.run([KWS_MAIN, "40", str(chunk), model_path, wav], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [line.split() for line in r.stdout.strip().splitlines()]
    got = np.array([[float(v) for v in w[3:]] for w in rows], np.float32)
    feats = Fbank(num_bins=40)(torch.from_numpy(pcm.astype(np.float32))[None].to("cuda"))
    m = build(cfg, sd)
    cache, ys = None, []
    for t in range(0, feats.size(1), chunk):
        y, cache = m(feats[:, t:t + chunk].contiguous(), cache)
        ys.append(y)
    want = torch.cat(ys, 1)[0].cpu().numpy()
    assert got.shape == want.shape == (1 + (40000 - 400) // 160, cfg["output_dim"])
    assert float(np.abs(got - want).max()) <= 1e-4
    golden = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kws_main_16k_ds_tcn_h64.txt")).read()
    assert r.stdout == golden
