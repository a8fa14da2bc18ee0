#!/usr/bin/env python3
"""Generate tests/golden/ctc_kws_golden.npz by executing the reference's own CTC decode: ``ctc_prefix_beam_search`` of
wekws/model/loss.py with score_ctc.py's per-utterance detection loop (offline), and ``KeyWordSpotter.forward`` /
``reset`` / ``reset_all`` of wekws/bin/stream_kws_ctc.py (streaming).  Build container only:

    WEKWS_REFERENCE=<reference checkout> python tests/golden/make_ctc_kws_golden.py

The spotter is built with ``object.__new__`` (no checkpoint, no token files); its ``accept_wave`` and ``model`` return
seeded chunks, and the posteriors its own ``logits.softmax(2)`` computes are recorded as the decoder input.  Results
are stored as JSON with every float as ``float.hex`` (bit-exact), inputs as float32 arrays ``off/<case>`` / ``str/<case>/<chunk>``.
"""
from __future__ import annotations

import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference():
    """(loss.ctc_prefix_beam_search, stream_kws_ctc module).  Stubs the spotter's PCM / lexicon imports."""
    ref = os.environ.get("WEKWS_REFERENCE")
    if not ref:
        sys.exit("set WEKWS_REFERENCE to the reference checkout")
    if ref not in sys.path:
        sys.path.insert(0, ref)
    for name in ("librosa", "torchaudio", "torchaudio.compliance", "torchaudio.compliance.kaldi"):
        sys.modules.setdefault(name, types.ModuleType(name))
    ml = types.ModuleType("tools.make_list")
    for name in ("query_token_set", "read_lexicon", "read_token"):
        setattr(ml, name, lambda *a, **k: None)
    sys.modules.setdefault("tools", types.ModuleType("tools"))
    sys.modules["tools.make_list"] = ml
    from wekws.model.loss import ctc_prefix_beam_search
    import wekws.bin.stream_kws_ctc as skc
    return ctc_prefix_beam_search, skc


def h(x: float) -> str:
    return float(x).hex()


def beam_json(hyps):
    """loss.py's return value: [(prefix, score, nodes)]."""
    return [[list(p), h(s), [[n["token"], n["frame"], h(n["prob"])] for n in nodes]] for p, s, nodes in hyps]


def cur_hyps_json(cur):
    return [[list(p), h(pb), h(pnb), [[n["token"], n["frame"], h(n["prob"])] for n in nodes]] for p, (pb, pnb, nodes) in cur]


def ref_offline(search, is_sublist, probs, length, keywords, tokenset, score_beam, path_beam):
    """score_ctc.py:183-236 around the reference's search (the loop itself is inline in score_ctc's main)."""
    hyps = search(torch.from_numpy(probs[:length]), torch.tensor([length]), tokenset, score_beam, path_beam)
    hit, hit_score, start, end = None, 1.0, 0, 0
    for prefix_ids, _, prefix_nodes in hyps:
        for k, lab in enumerate(keywords):
            offset = is_sublist(prefix_ids, lab)
            if offset != -1:
                hit = k
                start = prefix_nodes[offset]["frame"]
                end = prefix_nodes[offset + len(lab) - 1]["frame"]
                for idx in range(offset, offset + len(lab)):
                    hit_score *= prefix_nodes[idx]["prob"]
                break
        if hit is not None:
            hit_score = math.sqrt(hit_score)
            break
    return hyps, hit, hit_score, start, end


def make_spotter(skc, keywords, threshold, min_frames, max_frames, interval_frames, score_beam, path_beam, downsampling):
    kws = object.__new__(skc.KeyWordSpotter)
    torch.nn.Module.__init__(kws)
    kws.downsampling = downsampling
    kws.frame_shift = 10
    kws.resolution = kws.frame_shift / 1000
    kws.in_cache = torch.zeros(0, 0, 0)
    kws.score_beam, kws.path_beam = score_beam, path_beam
    kws.threshold, kws.min_frames, kws.max_frames, kws.interval_frames = threshold, min_frames, max_frames, interval_frames
    kws.keywords_token = {f"kw{k}": {"token_id": tuple(lab)} for k, lab in enumerate(keywords)}
    kws.keywords_idxset = {0} | {int(x) for lab in keywords for x in lab}
    kws.reset_all()
    return kws


def ref_stream_chunk(kws, logits: np.ndarray):
    """Drive KeyWordSpotter.forward with one chunk of logits (T, V); returns (the posteriors it decoded, its result)."""
    seen = {}

    def model(feats, cache):
        x = torch.from_numpy(logits).unsqueeze(0)
        seen["probs"] = x.softmax(2)[0].numpy().copy()
        return x, cache

    kws.accept_wave = lambda wave: torch.zeros(logits.shape[0], 1)
    kws.model = model
    res = kws.forward(b"")
    probs = seen.get("probs", np.zeros((0, logits.shape[1]), np.float32))
    return probs, res


def result_json(res):
    if not res:
        return {}
    return {k: (h(v) if isinstance(v, float) else v) for k, v in res.items()}


# ------------------------------------------------------------------------------------------------ inputs
def softmax(x):
    x = x - x.max(-1, keepdims=True)
    e = np.exp(x)
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def peaky_logits(rng, script, V, peak=7.0, noise=1.0):
    """One frame per script entry: the scripted token gets a boost over Gaussian distractors (a second one, smaller, for a
    tuple entry)."""
    # a dozen Gaussian distractors per frame over a flat floor: every other posterior of a row is the same value, which
    # keeps the recorded matrices small
    x = np.zeros((len(script), V), np.float32)
    d = rng.integers(0, V, size=(len(script), 12))
    np.put_along_axis(x, d, rng.normal(0.0, noise, size=d.shape).astype(np.float32), 1)
    for t, s in enumerate(script):
        for j, tok in enumerate(s if isinstance(s, tuple) else (s,)):
            x[t, tok] += peak - 2.5 * j
    top = np.argsort(-x, axis=1)[:, :9]          # un-quantise the places the first beam looks at: no exact ties there
    np.put_along_axis(x, top, np.take_along_axis(x, top, 1) + rng.uniform(0, 1 / 64, top.shape).astype(np.float32), 1)
    return x


def keyword_script(rng, keywords, T, p_kw=0.5):
    """Blank-dominated frames with keyword utterances (3-6 frames per token) at random places."""
    out = []
    while len(out) < T:
        if rng.random() < p_kw:
            lab = keywords[rng.integers(len(keywords))]
            for tok in lab:
                out += [int(tok)] * int(rng.integers(2, 6))
                out += [0] * int(rng.integers(0, 3))
        else:
            out += [0] * int(rng.integers(3, 15))
        if rng.random() < 0.3:
            out.append((0, int(rng.integers(1, 20))))
    return out[:T]


def no_ties(probs, k):
    """The documented deviation: exact ties inside the top-k (or at its k-th place) among values that survive the 0.05
    filter have no reference order; no golden frame holds one."""
    for row in probs.reshape(-1, probs.shape[-1]):
        top = np.sort(row[~np.isnan(row)])[::-1][:k + 1]
        v = top[top > 0.05]
        assert len(np.unique(v)) == len(v), "exact tie among surviving posteriors"


def rows(*frames, V):
    """Explicit posteriors: frames of {token: prob}; the remaining mass spread over the rest (below 0.05 each)."""
    out = np.zeros((len(frames), V), np.float32)
    for t, f in enumerate(frames):
        rest = [i for i in range(V) if i not in f]
        left = max(0.0, 1.0 - sum(f.values()))
        for i in rest:
            out[t, i] = left / len(rest) if rest else 0.0
        for i, p in f.items():
            out[t, i] = p
    return out


def offline_cases(rng):
    """(name, probs (B, T, V), lengths, keywords, tokenset or None, score_beam, path_beam)."""
    cs = []
    # 1. shared node records
    cs.append(("shared_nodes", rows({1: .6, 0: .4}, {2: .5, 1: .45}, {1: .9}, V=3)[None], [3], [(1, 2)], None, 3, 20))
    # 2. insertion-order ties of equal scores
    cs.append(("score_tie", rows({1: .5, 2: .3, 0: .2}, {2: .5, 1: .3, 0: .2}, V=3)[None], [2], [(1, 2)], None, 2, 20))
    # 4. the beam empties for good
    cs.append(("beam_empties", rows(*([{1: .06}] * 6 + [{1: .9}, {0: .9}]), V=20)[None], [8], [(1,)], None, 3, 20))
    # 5. is_sublist: a keyword at the very end of a longer prefix is missed, at the start found
    cs.append(("sublist_end", rows({9: .9}, {0: .9}, {1: .9}, {0: .9}, {2: .9}, V=20)[None], [5], [(1, 2)], None, 3, 1))
    cs.append(("sublist_start", rows({1: .9}, {0: .9}, {2: .9}, {0: .9}, {9: .9}, V=20)[None], [5], [(1, 2)], None, 3, 1))
    # 8. the token set filters after the top-k of the whole row
    cs.append(("tokenset_after_topk", rows({5: .4, 6: .3, 1: .2}, {0: .5, 7: .3, 2: .15}, V=20)[None], [2],
               [(1, 2)], {0, 1, 2}, 3, 20))
    # NaN: ranks above every number, takes a top-k place, is dropped
    nan = rows({1: .6, 0: .3}, {0: .7, 1: .2}, {2: .6, 0: .3}, V=8)
    nan[1, 5] = np.nan
    cs.append(("nan_place", nan[None], [3], [(1, 2)], None, 3, 20))
    alln = rows({1: .6, 0: .3}, {0: .7}, {2: .6, 0: .3}, V=8)
    alln[1, :] = np.nan
    cs.append(("nan_row", alln[None], [3], [(1, 2)], None, 3, 20))
    # seeded peaky posteriors over the three vocabulary sizes, padded batches, several beams
    for V, B, T, sb, pb, ts in ((20, 6, 40, 3, 20, True), (20, 4, 30, 8, 64, False), (300, 3, 50, 3, 20, True),
                                (300, 2, 40, 5, 4, False), (2599, 1, 98, 3, 20, True), (2599, 1, 40, 8, 20, False)):
        kws = [tuple(int(x) for x in rng.choice(np.arange(1, min(V, 40)), size=int(rng.integers(2, 5)), replace=False))
               for _ in range(3)]
        kws[2] = kws[0][:1] + kws[2][1:]           # keywords that share tokens
        x = np.stack([peaky_logits(rng, keyword_script(rng, kws, T), V, peak=float(rng.uniform(3, 8)),
                                   noise=float(rng.uniform(.5, 2))) for _ in range(B)])
        lengths = [T] + [int(rng.integers(0, T + 1)) for _ in range(B - 1)]
        cs.append((f"peaky_V{V}_sb{sb}_pb{pb}", softmax(x), lengths, kws, ({0} | {t for k in kws for t in k}) if ts else None,
                   sb, pb))
    return cs


def stream_cases(rng):
    """(name, dict(keywords, threshold, min_frames, max_frames, interval_frames, score_beam, path_beam, downsampling),
    ops: list of ('chunk', logits (T, V)) / ('reset',) / ('reset_all',))."""
    cs = []

    def chunks(x, sizes):
        ops, t = [], 0
        for n in sizes:
            ops.append(("chunk", x[t:t + n]))
            t += n
        return ops

    def cfg(kws, **kw):
        c = dict(keywords=kws, threshold=0.0, min_frames=5, max_frames=250, interval_frames=50, score_beam=3, path_beam=20,
                 downsampling=1)
        c.update(kw)
        return c

    kw2 = [(3, 4, 5), (3, 6)]
    # activation (then the rest of the chunk is skipped), a second keyword inside the interval, after it
    script = [0] * 5 + [3] * 4 + [0] * 2 + [4] * 4 + [5] * 4 + [0] * 10 + [3] * 3 + [6] * 3 + [0] * 70 + [3] * 3 + [6] * 4 + [0] * 20
    x = peaky_logits(rng, script, 20)
    cs.append(("activate_interval", cfg(kw2), chunks(x, [30] * (len(script) // 30) + [len(script) % 30])))
    # min / max duration
    cs.append(("too_short", cfg(kw2, min_frames=20), chunks(x, [30, 30, 30, 40])))
    cs.append(("too_long", cfg(kw2, max_frames=6), chunks(x, [30, 30, 30, 40])))
    # 6. a never-reached threshold: hit_score is multiplied every frame a keyword is found
    cs.append(("score_carried", cfg(kw2, threshold=2.0), chunks(x, [30, 30, 30, 40])))
    # aging reset (max_frames small) and a long prefix without keyword
    y = peaky_logits(rng, keyword_script(rng, kw2, 200, p_kw=.3), 20)
    cs.append(("aging", cfg(kw2, max_frames=25, threshold=2.0), chunks(y, [30] * 6 + [20])))
    # 1-frame and 0-frame chunks, downsampling 3
    cs.append(("tiny_chunks_ds3", cfg(kw2, downsampling=3), chunks(x, [1, 0, 1, 2, 0, 5, 1, 30, 1, 60, 30])))
    cs.append(("ds3", cfg(kw2, downsampling=3, threshold=.5), chunks(x, [30] * 4 + [len(script) - 120])))
    # 4. the beam empties for good in streaming (no aging check afterwards)
    z = np.log(np.maximum(rows(*([{3: .06}] * 8 + [{3: .9}, {4: .9}]), V=20), 1e-30))
    cs.append(("beam_empties", cfg(kw2), chunks(z, [4, 4, 2])))
    # reset / reset_all between chunks
    ops = chunks(x[:60], [30, 30]) + [("reset",)] + chunks(x[60:120], [30, 30]) + [("reset_all",)] + chunks(x[120:], [30, 40])
    cs.append(("resets", cfg(kw2, threshold=.3), ops))
    # large vocabulary, peaky, several configurations
    for V, sb, pb, ds, n in ((300, 3, 20, 1, 150), (2599, 3, 20, 1, 60), (2599, 5, 8, 3, 30), (20, 8, 64, 1, 200)):
        kws = [tuple(int(x) for x in rng.choice(np.arange(1, min(V, 40)), size=int(rng.integers(2, 4)), replace=False))
               for _ in range(3)]
        kws[1] = kws[0][:1] + kws[1][1:]
        x = peaky_logits(rng, keyword_script(rng, kws, n), V, peak=float(rng.uniform(4, 8)))
        sizes, left = [], n
        while left > 0:
            sizes.append(min(left, int(rng.integers(0, 40))))
            left -= sizes[-1]
        cs.append((f"peaky_V{V}_sb{sb}_pb{pb}_ds{ds}", cfg(kws, threshold=float(rng.uniform(0, .6)), score_beam=sb,
                                                            path_beam=pb, downsampling=ds, max_frames=int(rng.integers(40, 120))),
                   chunks(x, sizes)))
    return cs


def run_offline(search, is_sublist, case):
    name, probs, lengths, kws, ts, sb, pb = case
    no_ties(probs, sb)
    out = []
    for b in range(probs.shape[0]):
        hyps, hit, score, start, end = ref_offline(search, is_sublist, probs[b], lengths[b], kws, ts, sb, pb)
        out.append(dict(beam=beam_json(hyps), hit=hit, score=h(score), start=start, end=end))
    return out


def run_stream(skc, case):
    name, c, ops = case
    kws = make_spotter(skc, c["keywords"], c["threshold"], c["min_frames"], c["max_frames"], c["interval_frames"],
                       c["score_beam"], c["path_beam"], c["downsampling"])
    inputs, steps = [], []
    for op in ops:
        if op[0] == "chunk":
            probs, res = ref_stream_chunk(kws, op[1])
            no_ties(probs, c["score_beam"])
            inputs.append(probs)
            steps.append(dict(op="chunk", result=result_json(res), hit_score=h(kws.hit_score),
                              total_frames=kws.total_frames, last_active_pos=kws.last_active_pos,
                              beam=cur_hyps_json(kws.cur_hyps)))
        else:
            getattr(kws, op[0])()
            steps.append(dict(op=op[0]))
    return inputs, steps


def main():
    search, skc = load_reference()
    rng = np.random.default_rng(20261015)
    arrays, meta = {}, {"offline": [], "stream": []}
    for case in offline_cases(rng):
        name, probs, lengths, kws, ts, sb, pb = case
        arrays[f"off/{name}"] = probs
        meta["offline"].append(dict(name=name, lengths=lengths, keywords=[list(k) for k in kws],
                                    tokenset=None if ts is None else sorted(ts), score_beam=sb, path_beam=pb,
                                    expect=run_offline(search, skc.is_sublist, case)))
    for case in stream_cases(rng):
        name, c, _ = case
        inputs, steps = run_stream(skc, case)
        for i, p in enumerate(inputs):
            arrays[f"str/{name}/{i}"] = p
        meta["stream"].append(dict(name=name, config={**c, "keywords": [list(k) for k in c["keywords"]]}, steps=steps))
    arrays["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "ctc_kws_golden.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes;", len(meta["offline"]), "offline,", len(meta["stream"]), "stream cases")


if __name__ == "__main__":
    main()
