"""Host restatement of the CTC prefix beam search and keyword detection that wekws_amd.ctc runs on the device.

The behaviour restated is the reference's (wekws/model/loss.py:206-312 for the offline search, wekws/bin/score_ctc.py:183-236
for the per-utterance detection, wekws/bin/stream_kws_ctc.py:106-530 for the streaming spotter), written from the
semantics rather than the source.  The points a straightforward implementation gets wrong:

- a path node is a record with identity.  Hypotheses hold their own node lists, but the lists share node records, and the
  repeated-token update writes through the record, so every hypothesis holding it sees the new frame / prob.
- hypotheses are merged in first-touch order and the prune is a stable descending sort, so equal scores keep that order.
- probabilities are Python floats (f64); every update is evaluated left to right, one rounding per operation.
- the beam may become empty for good, and is_sublist never finds a keyword that ends the last place of a longer prefix.

Two documented deviations: exact ties inside the first-beam top-k go lower index first, and a frame
holding +-Inf fails its stream with EINVAL (NaN ranks above every number and is then dropped by the 0.05 filter)."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np

EINVAL = -1
ECAPACITY = -5


class Node:
    __slots__ = ("token", "frame", "prob")

    def __init__(self, token: int, frame: int, prob: float):
        self.token, self.frame, self.prob = token, frame, prob


class Hyp:
    """One beam entry: the prefix, the two path probabilities and the (shared) node records of its tokens."""
    __slots__ = ("prefix", "pb", "pnb", "nodes")

    def __init__(self, prefix: tuple, pb: float, pnb: float, nodes: list):
        self.prefix, self.pb, self.pnb, self.nodes = prefix, pb, pnb, nodes

    def score(self) -> float:
        return self.pb + self.pnb


def initial_beam() -> List[Hyp]:
    return [Hyp((), 1.0, 0.0, [])]


def first_beam(row: np.ndarray, score_beam: int, tokenset) -> List[int]:
    """Tokens of one frame that the search expands, best first: top `score_beam` of the whole row (NaN above every
    number, equal values lower index first), then prob > 0.05, then membership in the token set."""
    row = np.asarray(row, dtype=np.float32)
    nan = np.isnan(row)
    num = np.flatnonzero(~nan)
    order = np.concatenate([np.flatnonzero(nan), num[np.argsort(-row[num], kind="stable")]])
    keep = []
    for i in order[:score_beam].tolist():
        p = float(row[i])
        if p > 0.05 and (tokenset is None or i in tokenset):
            keep.append(i)
    return keep


def has_inf(row) -> bool:
    return bool(np.isinf(np.asarray(row, dtype=np.float32)).any())


def search_step(beam: List[Hyp], row: np.ndarray, t: int, score_beam: int, path_beam: int, tokenset) -> List[Hyp]:
    """One frame.  Returns the new beam (the old one, untouched, when no token survives the first prune)."""
    tokens = first_beam(row, score_beam, tokenset)
    if not tokens:
        return beam
    merged: Dict[tuple, Hyp] = {}      # insertion order == first-touch order

    def touch(prefix: tuple) -> Hyp:
        h = merged.get(prefix)
        if h is None:
            h = merged[prefix] = Hyp(prefix, 0.0, 0.0, [])
        return h

    for s in tokens:
        ps = float(row[s])
        for cur in beam:
            last = cur.prefix[-1] if cur.prefix else None
            if s == 0:
                h = touch(cur.prefix)
                h.pb = h.pb + cur.pb * ps + cur.pnb * ps
                h.nodes = list(cur.nodes)
            elif s == last:
                if abs(cur.pnb) > 1e-6:
                    h = touch(cur.prefix)
                    h.pnb = h.pnb + cur.pnb * ps
                    h.nodes = list(cur.nodes)
                    tail = h.nodes[-1]
                    if ps > tail.prob:                 # written through the shared record
                        tail.prob, tail.frame = ps, t
                if abs(cur.pb) > 1e-6:
                    h = touch(cur.prefix + (s,))
                    h.pnb = h.pnb + cur.pb * ps
                    h.nodes = list(cur.nodes) + [Node(s, t, ps)]
            else:
                fresh = (cur.prefix + (s,)) not in merged
                h = touch(cur.prefix + (s,))
                if not fresh:
                    if ps > h.nodes[-1].prob:          # the entry's own list: replace its last record by a new one
                        h.nodes.pop()
                        h.nodes.append(Node(s, t, ps))
                else:
                    h.nodes = list(cur.nodes) + [Node(s, t, ps)]
                h.pnb = h.pnb + cur.pb * ps + cur.pnb * ps
    ranked = sorted(merged.values(), key=Hyp.score, reverse=True)
    return ranked[:path_beam]


def is_sublist(main: Sequence[int], check: Sequence[int]) -> int:
    """First offset of `check` in `main`; an occurrence that ends at the last place of a longer `main` is not found."""
    main, check = tuple(main), tuple(check)
    if len(main) < len(check):
        return -1
    if len(main) == len(check):
        return 0 if main == check else -1
    for i in range(len(main) - len(check)):
        if main[i:i + len(check)] == check:
            return i
    return -1


def detect(beam: List[Hyp], keywords: Sequence[Sequence[int]], hit_score: float):
    """Keyword search over a beam: hypotheses in beam order, keywords in insertion order, the first hit wins.  Returns
    (keyword index or None, hit_score after the update, start frame, end frame)."""
    for h in beam:
        for k, lab in enumerate(keywords):
            off = is_sublist(h.prefix, lab)
            if off != -1:
                for n in h.nodes[off:off + len(lab)]:
                    hit_score *= n.prob
                return k, math.sqrt(hit_score), h.nodes[off].frame, h.nodes[off + len(lab) - 1].frame
    return None, hit_score, 0, 0


def prefix_beam_search(probs: np.ndarray, score_beam: int = 3, path_beam: int = 20, tokenset=None):
    """Offline search over one utterance's (T, V) posteriors.  Returns (beam, status)."""
    beam = initial_beam()
    for t in range(probs.shape[0]):
        if has_inf(probs[t]):
            return beam, EINVAL
        beam = search_step(beam, probs[t], t, score_beam, path_beam, tokenset)
    return beam, 0


def keyword_search(probs: np.ndarray, keywords, score_beam: int = 3, path_beam: int = 20, tokenset=None):
    """score_ctc's per-utterance loop: (keyword index or None, hit score, start, end, status, beam)."""
    beam, status = prefix_beam_search(probs, score_beam, path_beam, tokenset)
    k, score, start, end = detect(beam, keywords, 1.0)
    return k, score, start, end, status, beam


def default_tokenset(keywords) -> set:
    ts = {0}
    for lab in keywords:
        ts.update(int(x) for x in lab)
    return ts


class Spotter:
    """One stream of the streaming spotter (the post-model part of KeyWordSpotter.forward, with reset / reset_all)."""

    def __init__(self, keywords, threshold, min_frames=5, max_frames=250, interval_frames=50, score_beam=3,
                 path_beam=20, downsampling=1, capacity=None):
        self.keywords = [tuple(int(x) for x in k) for k in keywords]
        self.tokenset = default_tokenset(self.keywords)
        self.threshold, self.min_frames, self.max_frames = threshold, min_frames, max_frames
        self.interval_frames, self.score_beam, self.path_beam = interval_frames, score_beam, path_beam
        self.downsampling, self.capacity = downsampling, capacity
        self.reset_all()

    def reset(self):
        self.beam = initial_beam()
        self.activated = False
        self.hit_score = 1.0
        self.status = 0

    def reset_all(self):
        self.reset()
        self.total_frames = 0
        self.last_active_pos = -1
        self.result = None

    def step(self, probs: np.ndarray):
        """One chunk of (T, V) posteriors.  Returns None for an empty chunk (the reference's `{}`), else a record
        dict(state, keyword, start, end, score, hit) with frame numbers, plus `status`."""
        if probs.shape[0] == 0:
            return None
        if self.status:
            return dict(status=self.status, state=0, keyword=None, start=0, end=0, score=self.hit_score, hit=None)
        for t in range(probs.shape[0]):
            at = t * self.downsampling + self.total_frames
            if has_inf(probs[t]):
                self.status = EINVAL
                return dict(status=self.status, state=0, keyword=None, start=0, end=0, score=self.hit_score, hit=None)
            nb = search_step(self.beam, probs[t], at, self.score_beam, self.path_beam, self.tokenset)
            if self.capacity is not None and any(len(h.prefix) > self.capacity for h in nb):
                self.status = ECAPACITY
                return dict(status=self.status, state=0, keyword=None, start=0, end=0, score=self.hit_score, hit=None)
            self.beam = nb
            k, self.hit_score, start, end = detect(self.beam, self.keywords, self.hit_score)
            if k is not None and self.hit_score >= self.threshold and self.min_frames <= end - start <= self.max_frames \
                    and (self.last_active_pos == -1 or end - self.last_active_pos >= self.interval_frames):
                self.activated = True
                self.last_active_pos = end
            self.result = dict(status=0, state=1 if self.activated else 0, keyword=k, start=start, end=end,
                               score=self.hit_score, hit=k)
            if self.activated:
                self.reset()
                break
        self.total_frames += probs.shape[0] * self.downsampling
        if self.beam and self.beam[0].prefix:
            if self.total_frames - int(self.beam[0].nodes[0].frame) > self.max_frames:
                self.reset()
        return dict(self.result)


def as_result_dict(rec, keyword_names, frame_shift_ms=10):
    """A step record -> KeyWordSpotter.forward's result dict."""
    if rec is None:
        return {}
    res = frame_shift_ms / 1000
    on = rec["state"] == 1
    return {"state": 1 if on else 0, "keyword": keyword_names[rec["keyword"]] if on else None,
            "start": rec["start"] * res if on else None, "end": rec["end"] * res if on else None,
            "score": rec["score"] if on else None}


def beam_as_reference(beam: List[Hyp]):
    """The reference's return shape: [(prefix, pb + pnb, [dict(token, frame, prob), ...]), ...]."""
    return [(h.prefix, h.score(), [dict(token=n.token, frame=n.frame, prob=n.prob) for n in h.nodes]) for h in beam]
