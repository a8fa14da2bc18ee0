"""Loader of tests/golden/ctc_kws_golden.npz (written by tests/golden/make_ctc_kws_golden.py from the reference) and
the conversions between its JSON records and the oracle's / the device's values.  Floats are compared as bits."""
from __future__ import annotations

import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctc_kws_golden.npz")


def load():
    z = np.load(PATH)
    meta = json.loads(str(z["meta"]))
    return z, meta


def fx(s: str) -> float:
    return float.fromhex(s)


def beam_expect(hyps):
    """loss.py's [(prefix, score, nodes)] JSON -> [(prefix tuple, score, [(token, frame, prob)])]."""
    return [(tuple(p), fx(s), [(t, f, fx(pr)) for t, f, pr in nodes]) for p, s, nodes in hyps]


def cur_hyps_expect(hyps):
    """cur_hyps JSON -> [(prefix, pb, pnb, [(token, frame, prob)])]."""
    return [(tuple(p), fx(pb), fx(pnb), [(t, f, fx(pr)) for t, f, pr in nodes]) for p, pb, pnb, nodes in hyps]


def result_expect(res):
    return {k: (fx(v) if isinstance(v, str) and k == "score" or k in ("start", "end") and isinstance(v, str) else v)
            for k, v in res.items()}


def oracle_beam(beam):
    return [(h.prefix, h.score(), [(n.token, n.frame, n.prob) for n in h.nodes]) for h in beam]


def oracle_cur_hyps(beam):
    return [(h.prefix, h.pb, h.pnb, [(n.token, n.frame, n.prob) for n in h.nodes]) for h in beam]
