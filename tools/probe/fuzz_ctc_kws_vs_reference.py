#!/usr/bin/env python3
"""The CTC decode oracle (tests/ctc_kws_ref.py) against the reference's own functions on random seeds: the offline
search + score_ctc detection, and KeyWordSpotter.forward / reset / reset_all driven with random chunkings.  Build
container only (needs the reference checkout):

    WEKWS_REFERENCE=<reference checkout> python tools/probe/fuzz_ctc_kws_vs_reference.py [first_seed] [n_seeds]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import ctc_kws_golden as G  # noqa: E402
from tests import ctc_kws_ref as R  # noqa: E402
from tests.golden import make_ctc_kws_golden as M  # noqa: E402


def one(seed, search, skc):
    rng = np.random.default_rng(seed)
    V = int(rng.choice([20, 40, 300]))
    kws = [tuple(int(x) for x in rng.choice(np.arange(1, min(V, 12)), int(rng.integers(1, 4)), replace=False))
           for _ in range(int(rng.integers(1, 4)))]
    sb, pb = int(rng.integers(1, 9)), int(rng.choice([1, 3, 20, 64]))
    # offline
    T = int(rng.integers(0, 60))
    x = M.softmax(M.peaky_logits(rng, M.keyword_script(rng, kws, T), V, float(rng.uniform(2, 8)), float(rng.uniform(.3, 2))))
    try:
        M.no_ties(x, sb)
    except AssertionError:
        return "tie"
    ts = R.default_tokenset(kws) if rng.random() < .7 else None
    hyps, hit, score, start, end = M.ref_offline(search, skc.is_sublist, x, T, kws, ts, sb, pb)
    k, s2, st2, en2, _, beam = R.keyword_search(x, kws, sb, pb, ts)
    assert G.oracle_beam(beam) == G.beam_expect(M.beam_json(hyps)), seed
    assert (k, s2, st2, en2) == (hit, score, start, end), seed
    # streaming
    c = dict(threshold=float(rng.uniform(0, .8)), min_frames=int(rng.integers(0, 8)), max_frames=int(rng.integers(10, 100)),
             interval_frames=int(rng.integers(0, 60)), downsampling=int(rng.choice([1, 2, 3])))
    ref = M.make_spotter(skc, kws, c["threshold"], c["min_frames"], c["max_frames"], c["interval_frames"], sb, pb,
                         c["downsampling"])
    orc = R.Spotter(kws, c["threshold"], c["min_frames"], c["max_frames"], c["interval_frames"], sb, pb, c["downsampling"])
    for _ in range(int(rng.integers(1, 12))):
        r = rng.random()
        if r < .08:
            ref.reset(); orc.reset(); continue
        if r < .12:
            ref.reset_all(); orc.reset_all(); continue
        n = int(rng.integers(0, 40))
        lg = M.peaky_logits(rng, M.keyword_script(rng, kws, n), V, float(rng.uniform(2, 8)))
        probs, res = M.ref_stream_chunk(ref, lg)
        try:
            M.no_ties(probs, sb)
        except AssertionError:
            return "tie"
        got = R.as_result_dict(orc.step(probs), [f"kw{i}" for i in range(len(kws))])
        assert got == res, (seed, got, res)
        assert orc.hit_score == ref.hit_score and orc.total_frames == ref.total_frames, seed
        assert G.oracle_cur_hyps(orc.beam) == G.cur_hyps_expect(M.cur_hyps_json(ref.cur_hyps)), seed
    return "ok"


def main():
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    search, skc = M.load_reference()
    counts = {}
    for seed in range(first, first + n):
        r = one(seed, search, skc)
        counts[r] = counts.get(r, 0) + 1
    print(f"seeds {first} .. {first + n - 1}: {counts}, 0 failures")


if __name__ == "__main__":
    main()
