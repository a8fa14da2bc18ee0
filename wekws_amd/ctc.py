"""Device side of the CTC keyword decoder.

- ``softmax_topk`` / ``first_beam_prune``: the first beam prune of ``ctc_prefix_beam_search`` (wekws/model/loss.py:236-251)
  computed from the LOGITS in one kernel (``wekws_hip_softmax_topk``).
- ``ctc_prefix_beam_search`` / ``keyword_search`` / ``StreamingKeywordSpotter``: the whole decode -- the prefix beam search
  of loss.py:206-312, score_ctc's detection loop and the streaming ``KeyWordSpotter`` of wekws/bin/stream_kws_ctc.py --
  on the device for a batch of utterances or thousands of streams (``wekws_hip_ctc_kws_*``, csrc/ctc_kws.hip.h), bit-identical
  to the reference given the same float32 posteriors.  The host receives one small result record per stream and call.
  Intended use: ``probs, cache = model.forward_softmax(chunk, cache); res = spotter.step(probs)``.
- keyword sets: every stream of a ``StreamingKeywordSpotter`` (``add_keywords`` / ``assign`` / ``drop_keywords``) and every
  row of ``keyword_search_sets`` may have its own keywords, token set and threshold (``wekws_hip_ctc_kws_add_set`` / ``_assign``
  / ``_drop_set`` / ``_search_sets``, csrc/ctc_kws_sets.h) -- ``KeyWordSpotter.set_keywords`` per stream instead of per object."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import torch

from wekws_amd import _capi


def softmax_topk(logits: torch.Tensor, k: int = 3) -> Tuple[torch.Tensor, torch.Tensor]:
    """(..., K) float32 logits on a ROCm device -> (probs (..., k) float32, index (..., k) int64), i.e.
    ``logits.softmax(-1).topk(k)`` without materialising the softmax.  Equal values: lower index first."""
    if not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() < 1:
        raise ValueError("logits must be a float32 tensor on a ROCm device (no CPU fallback)")
    lib = _capi.load()
    x = logits.contiguous()
    K = int(x.size(-1))
    rows = x.numel() // K if K else 0
    probs = torch.empty(x.shape[:-1] + (k,), dtype=torch.float32, device=x.device)
    idx = torch.empty(x.shape[:-1] + (k,), dtype=torch.int32, device=x.device)
    if rows:
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _capi.check(lib.wekws_hip_softmax_topk(x.data_ptr(), rows, K, int(k), probs.data_ptr(), idx.data_ptr(),
                                               ctypes.c_void_p(stream)), "wekws_hip_softmax_topk")
    return probs, idx.to(torch.int64)


def first_beam_prune(logits: torch.Tensor, score_beam_size: int = 3, keywords_tokenset=None, min_prob: float = 0.05):
    """Per frame of a (T, K) logit matrix: the (prob, token) pairs that survive loss.py:236-251 -- top
    ``score_beam_size`` posteriors, prob > 0.05, token in ``keywords_tokenset`` if given.  Returns a list (one entry per
    frame) of lists of (prob, token); only T * k values cross PCIe."""
    probs, idx = softmax_topk(logits, score_beam_size)
    probs, idx = probs.cpu().tolist(), idx.cpu().tolist()
    out = []
    for pr, ix in zip(probs, idx):
        out.append([(p, i) for p, i in zip(pr, ix)
                    if p > min_prob and i >= 0 and (keywords_tokenset is None or i in keywords_tokenset)])
    return out


def _cuda_f32(probs: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(probs, torch.Tensor) or not probs.is_cuda or probs.dtype != torch.float32 or probs.dim() != 3:
        raise ValueError(f"{what}: probs must be a (B, T, V) float32 tensor on a ROCm device (no CPU fallback)")
    return probs.contiguous()


def _keyword_lists(keywords) -> Tuple[List[str], List[Tuple[int, ...]]]:
    """dict name -> token ids (insertion order), or a sequence of token-id sequences (named by their index)."""
    if isinstance(keywords, dict):
        names, toks = list(keywords), [tuple(int(x) for x in v) for v in keywords.values()]
    else:
        toks = [tuple(int(x) for x in v) for v in keywords]
        names = list(range(len(toks)))
    return names, toks


class _Handle:
    """One ``wekws_hip_ctc_kws`` object."""

    def __init__(self, device: int, vocab: int, keywords: Sequence[Tuple[int, ...]], tokenset, score_beam: int,
                 path_beam: int, threshold: float = 0.0, min_frames: int = 5, max_frames: int = 250,
                 interval_frames: int = 50, downsampling: int = 1, max_streams: int = 0, prefix_capacity: int = 1):
        self.lib = _capi.load()
        self.path_beam = int(path_beam)
        flat = np.array([t for k in keywords for t in k] or [0], np.int32)
        offs = np.array([0] + list(np.cumsum([len(k) for k in keywords])), np.int32)
        ts = None if tokenset is None else np.array(sorted(int(x) for x in tokenset) or [0], np.int32)
        d = _capi.CtcKwsDesc(vocab=int(vocab), score_beam=int(score_beam), path_beam=int(path_beam),
                             num_keywords=len(keywords), keyword_tokens=flat.ctypes.data, keyword_offsets=offs.ctypes.data,
                             token_set=None if ts is None else ts.ctypes.data,
                             token_set_len=0 if tokenset is None else len(tokenset), min_frames=int(min_frames),
                             max_frames=int(max_frames), interval_frames=int(interval_frames),
                             downsampling=int(downsampling), max_streams=int(max_streams),
                             prefix_capacity=int(prefix_capacity), device=int(device), threshold=float(threshold))
        h = ctypes.c_void_p()
        _capi.check(self.lib.wekws_hip_ctc_kws_create(ctypes.byref(d), ctypes.byref(h)), "wekws_hip_ctc_kws_create")
        self.h = h

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            self.lib.wekws_hip_ctc_kws_destroy(h)

    def beam_bytes(self, cap: int) -> int:
        return int(self.lib.wekws_hip_ctc_kws_beam_bytes(self.h, int(cap)))

    def add_set(self, keywords: Sequence[Tuple[int, ...]], tokenset, threshold: float, stream: int) -> int:
        """Register a keyword set (wekws_hip_ctc_kws_add_set); tokenset None = no first-beam set.  Returns its id."""
        flat = np.array([t for k in keywords for t in k] or [0], np.int32)
        offs = np.array([0] + list(np.cumsum([len(k) for k in keywords])), np.int32)
        ts = None if tokenset is None else np.array(sorted(int(x) for x in tokenset) or [0], np.int32)
        out = ctypes.c_int32(-1)
        _capi.check(self.lib.wekws_hip_ctc_kws_add_set(self.h, flat.ctypes.data, offs.ctypes.data, len(keywords),
                                                       None if ts is None else ts.ctypes.data,
                                                       0 if tokenset is None else len(tokenset), float(threshold),
                                                       ctypes.byref(out), ctypes.c_void_p(stream)),
                    "wekws_hip_ctc_kws_add_set")
        return int(out.value)

    def drop_set(self, set_id: int, stream: int) -> None:
        _capi.check(self.lib.wekws_hip_ctc_kws_drop_set(self.h, int(set_id), ctypes.c_void_p(stream)),
                    "wekws_hip_ctc_kws_drop_set")

    def assign(self, ids: Sequence[int], sets: Sequence[int], stream: int) -> None:
        a, b = np.array(list(ids), np.int32), np.array(list(sets), np.int32)
        _capi.check(self.lib.wekws_hip_ctc_kws_assign(self.h, a.ctypes.data, b.ctypes.data, len(a), ctypes.c_void_p(stream)),
                    "wekws_hip_ctc_kws_assign")

    def decode_beam(self, raw: np.ndarray, cap: int):
        """One beam record -> [(prefix, pb, pnb, [(token, frame, prob), ...]), ...] in beam order."""
        PB = self.path_beam
        pbe = (PB + 1) & ~1
        pc = PB * cap
        cnt = int(raw[:4].view(np.int32)[0])
        lens = raw[8:8 + 4 * PB].view(np.int32)
        o = 8 + 4 * pbe
        pb = raw[o:o + 8 * PB].view(np.float64)
        pnb = raw[o + 8 * PB:o + 16 * PB].view(np.float64)
        o += 16 * PB
        tok = raw[o:o + 4 * pc].view(np.int32).reshape(PB, cap)
        fr = raw[o + 4 * pc:o + 8 * pc].view(np.int32).reshape(PB, cap)
        o += 8 * pc + 4 * (pc & 1)
        pr = raw[o:o + 8 * pc].view(np.float64).reshape(PB, cap)
        out = []
        for e in range(cnt):
            n = int(lens[e])
            out.append((tuple(int(x) for x in tok[e, :n]), float(pb[e]), float(pnb[e]),
                        [(int(tok[e, i]), int(fr[e, i]), float(pr[e, i])) for i in range(n)]))
        return out


def _results(res: torch.Tensor) -> np.ndarray:
    return np.frombuffer(res.cpu().numpy().tobytes(), dtype=np.dtype([("status", "<i4"), ("valid", "<i4"), ("state", "<i4"),
                                                                       ("keyword", "<i4"), ("start", "<i4"),
                                                                       ("end", "<i4"), ("score", "<f8")]))


def _search(probs, lengths, keywords, tokenset, score_beam_size, path_beam_size, want_beams: bool, more_sets=(),
            set_of_row=None):
    """One offline search.  ``more_sets``: (keywords, tokenset) pairs registered as sets 1, 2, ... beside the handle's own;
    ``set_of_row``: the set of every row (None: set 0)."""
    x = _cuda_f32(probs, "ctc decode")
    B, T, V = x.shape
    if V < 1:
        raise ValueError("ctc decode: the vocabulary is empty")
    dev = x.device
    if lengths is None:
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    else:
        lens = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).reshape(-1)
        if lens.numel() != B:
            raise ValueError(f"ctc decode: {lens.numel()} lengths for {B} utterances")
    hd = _Handle(dev.index or 0, V, keywords, tokenset, score_beam_size, path_beam_size)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for i, (kws, ts) in enumerate(more_sets):
        if hd.add_set(kws, ts, 0.0, stream) != i + 1:
            raise RuntimeError("ctc decode: keyword set ids out of order")
    rows = None
    if set_of_row is not None:
        rows = np.array([int(s) for s in set_of_row], np.int32)
        if rows.size != B or (B and (rows.min() < 0 or rows.max() > len(more_sets))):
            raise ValueError(f"ctc decode: set_of_row must hold {B} indices in 0..{len(more_sets)}")
    res = torch.empty((B, 32), dtype=torch.uint8, device=dev)
    cap = max(T, 1)
    bb = hd.beam_bytes(cap)
    beams = torch.empty((B, bb), dtype=torch.uint8, device=dev) if (want_beams and B) else None
    if B and rows is None:
        _capi.check(hd.lib.wekws_hip_ctc_kws_search(hd.h, x.data_ptr(), B, T, lens.data_ptr(), res.data_ptr(),
                                                     beams.data_ptr() if beams is not None else None,
                                                     ctypes.c_void_p(stream)), "wekws_hip_ctc_kws_search")
    elif B:
        _capi.check(hd.lib.wekws_hip_ctc_kws_search_sets(hd.h, x.data_ptr(), B, T, lens.data_ptr(), rows.ctypes.data,
                                                          res.data_ptr(), beams.data_ptr() if beams is not None else None,
                                                          ctypes.c_void_p(stream)), "wekws_hip_ctc_kws_search_sets")
    r = _results(res)
    for b in range(B):
        if r["status"][b] != 0:
            raise ValueError(f"ctc decode: utterance {b} failed with status {int(r['status'][b])} "
                             "(an infinite posterior, or a length outside 0..T)")
    raw = beams.cpu().numpy() if beams is not None else None
    return hd, r, raw, cap


def ctc_prefix_beam_search(probs: torch.Tensor, lengths=None, keywords_tokenset=None, score_beam_size: int = 3,
                           path_beam_size: int = 20):
    """loss.py's ``ctc_prefix_beam_search`` over a batch: probs (B, T, V) posteriors on the device, lengths (B) valid
    frames.  Returns, per utterance, the reference's n-best ``[(prefix, pb + pnb, [dict(token, frame, prob), ...]), ...]``."""
    hd, r, raw, cap = _search(probs, lengths, [], keywords_tokenset, score_beam_size, path_beam_size, True)
    out = []
    for b in range(len(r)):
        beam = hd.decode_beam(raw[b], cap)
        out.append([(p, pb + pnb, [dict(token=t, frame=f, prob=q) for t, f, q in nodes]) for p, pb, pnb, nodes in beam])
    return out


def keyword_search(probs: torch.Tensor, lengths, keywords, score_beam_size: int = 3, path_beam_size: int = 20):
    """score_ctc.py's per-utterance decision: the search with the keywords' token set (blank included), then the first
    keyword found in the n-best.  Returns per utterance ``(keyword or None, hit_score, start frame, end frame)``."""
    names, toks = _keyword_lists(keywords)
    tokenset = {0} | {t for k in toks for t in k}
    _, r, _, _ = _search(probs, lengths, toks, tokenset, score_beam_size, path_beam_size, False)
    return [(names[int(x["keyword"])] if x["state"] else None, float(x["score"]), int(x["start"]), int(x["end"]))
            for x in r]


def keyword_search_sets(probs: torch.Tensor, lengths, keyword_sets, set_of_row, score_beam_size: int = 3,
                        path_beam_size: int = 20):
    """``keyword_search`` with a keyword list per row, in one launch: ``keyword_sets`` is a sequence of keyword collections
    (each a dict or a sequence, as ``keyword_search`` takes one), ``set_of_row[b]`` the index of row b's.  Every set decodes
    with its own token set (blank included).  Returns per utterance ``(keyword or None, hit_score, start frame, end frame)``,
    the keyword named from the row's own set."""
    lists = [_keyword_lists(k) for k in keyword_sets]
    if not lists:
        raise ValueError("keyword_search_sets: no keyword set")
    sets = [(toks, {0} | {t for k in toks for t in k}) for _, toks in lists]
    which = [int(s) for s in set_of_row]
    _, r, _, _ = _search(probs, lengths, sets[0][0], sets[0][1], score_beam_size, path_beam_size, False, sets[1:], which)
    return [(lists[s][0][int(x["keyword"])] if x["state"] else None, float(x["score"]), int(x["start"]), int(x["end"]))
            for x, s in zip(r, which)]


class StreamingKeywordSpotter:
    """``KeyWordSpotter`` (wekws/bin/stream_kws_ctc.py) after the model, for ``num_streams`` streams on one device.

    ``step(probs, frames=None, streams=None)``: probs (B, T, V) posteriors on the device (``forward_softmax``'s output),
    row b continuing stream ``streams[b]`` (default: 0 .. B-1) with its first ``frames[b]`` frames (default T).  Returns,
    per row, ``KeyWordSpotter.forward``'s result dict (``{}`` for a row without frames); a stream that failed (an infinite
    posterior, a prefix beyond ``prefix_capacity``) returns ``{"status": code}`` until ``reset`` / ``reset_all``.

    Every stream may have its own keywords (``KeyWordSpotter.set_keywords``, one object per user, in the reference):
    ``add_keywords`` registers a keyword set beside the constructor's (set 0, where every stream starts), ``assign`` gives it
    to streams -- from its next frame an assigned stream is a fresh ``KeyWordSpotter`` built with that set --, ``drop_keywords``
    frees a set no stream uses.  The beams and ``min_frames`` / ``max_frames`` / ``interval_frames`` stay the spotter's."""

    def __init__(self, num_streams: int, keywords, threshold: float, min_frames: int = 5, max_frames: int = 250,
                 interval_frames: int = 50, score_beam: int = 3, path_beam: int = 20, downsampling: int = 1,
                 frame_shift_ms: float = 10, vocab: Optional[int] = None, prefix_capacity: Optional[int] = None,
                 device=None):
        self.names, toks = _keyword_lists(keywords)
        self.num_streams = int(num_streams)
        self.resolution = frame_shift_ms / 1000
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.vocab = vocab
        self._cfg = dict(keywords=toks, tokenset={0} | {t for k in toks for t in k}, score_beam=score_beam,
                         path_beam=path_beam, threshold=threshold, min_frames=min_frames, max_frames=max_frames,
                         interval_frames=interval_frames, downsampling=downsampling, max_streams=num_streams,
                         prefix_capacity=prefix_capacity or max(256, 2 * max_frames + 64))
        self._hd = None
        # host mirror of the keyword sets: id -> names, and the set of every stream
        self._set_names = {0: self.names}
        self._set_of = [0] * self.num_streams
        if vocab is not None:
            self._create(vocab)

    def _create(self, vocab: int):
        c = self._cfg
        self._hd = _Handle(self.device.index or 0, vocab, c["keywords"], c["tokenset"], c["score_beam"], c["path_beam"],
                           c["threshold"], c["min_frames"], c["max_frames"], c["interval_frames"], c["downsampling"],
                           c["max_streams"], c["prefix_capacity"])
        self.vocab = vocab

    def _id_list(self, streams, n: int) -> List[int]:
        ids = list(range(n)) if streams is None else [int(s) for s in (streams.tolist() if hasattr(streams, "tolist") else streams)]
        if len(ids) != n:
            raise ValueError(f"{len(ids)} stream ids for {n} rows")
        if len(set(ids)) != len(ids) or any(s < 0 or s >= self.num_streams for s in ids):
            raise ValueError(f"stream ids must be distinct and in 0..{self.num_streams - 1}")
        return ids

    def _ids(self, streams, n: int) -> torch.Tensor:
        return torch.tensor(self._id_list(streams, n), dtype=torch.int32, device=self.device)

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def add_keywords(self, keywords, threshold: Optional[float] = None, tokenset=None) -> int:
        """Register a keyword set: ``keywords`` a dict or a sequence as the constructor takes, ``threshold`` None = the
        spotter's own, ``tokenset`` None = the reference's ``{0} | tokens``.  Returns the set's id (>= 1)."""
        if self._hd is None:
            if self.vocab is None:
                raise ValueError("StreamingKeywordSpotter.add_keywords: the vocabulary is not known yet: pass vocab= to the "
                                 "constructor")
            self._create(self.vocab)
        names, toks = _keyword_lists(keywords)
        ts = {0} | {t for k in toks for t in k} if tokenset is None else {int(t) for t in tokenset}
        thr = self._cfg["threshold"] if threshold is None else threshold
        sid = self._hd.add_set(toks, ts, thr, self._stream())
        self._set_names[sid] = names
        return sid

    def assign(self, streams, set_id: int) -> None:
        """The streams (None: all) now use keyword set ``set_id`` and start over as by ``reset_all``."""
        set_id = int(set_id)
        if set_id not in self._set_names:
            raise ValueError(f"keyword set {set_id} is not registered")
        ids = self._id_list(streams, len(streams) if streams is not None else self.num_streams)
        if not ids:
            return
        if self._hd is None:
            if self.vocab is None:
                raise ValueError("StreamingKeywordSpotter.assign: the vocabulary is not known yet: pass vocab= to the constructor")
            self._create(self.vocab)
        self._hd.assign(ids, [set_id] * len(ids), self._stream())
        for s in ids:
            self._set_of[s] = set_id

    def drop_keywords(self, set_id: int) -> None:
        """Forget a keyword set no stream is assigned to; its id is handed out again."""
        set_id = int(set_id)
        if set_id == 0 or set_id not in self._set_names:
            raise ValueError(f"keyword set {set_id} is not registered" if set_id else "set 0 is the spotter's own")
        self._hd.drop_set(set_id, self._stream())
        del self._set_names[set_id]

    def keywords_of(self, stream: int) -> int:
        """The id of the stream's keyword set."""
        if not 0 <= int(stream) < self.num_streams:
            raise ValueError(f"stream id {stream} outside 0..{self.num_streams - 1}")
        return self._set_of[int(stream)]

    def step(self, probs: torch.Tensor, frames=None, streams=None) -> List[Dict]:
        recs, ids = self._step(probs, frames, streams)
        return [self._dict(r, s) for r, s in zip(recs, ids)]

    def _dict(self, r, stream: Optional[int] = None) -> Dict:
        """A result record as ``KeyWordSpotter.forward``'s dict; the keyword is named from the stream's own set."""
        if r["status"] != 0:
            return {"status": int(r["status"])}
        if not r["valid"]:
            return {}
        on = bool(r["state"])
        names = self.names if stream is None else self._set_names[self._set_of[stream]]
        return {"state": 1 if on else 0, "keyword": names[int(r["keyword"])] if on else None,
                "start": int(r["start"]) * self.resolution if on else None,
                "end": int(r["end"]) * self.resolution if on else None, "score": float(r["score"]) if on else None}

    def step_records(self, probs: torch.Tensor, frames=None, streams=None) -> np.ndarray:
        """``step`` returning the raw result records (status, valid, state, keyword, start, end, score) -- hit_score and
        the last detection included when the stream did not activate."""
        return self._step(probs, frames, streams)[0]

    def _step(self, probs: torch.Tensor, frames, streams) -> Tuple[np.ndarray, List[int]]:
        """The records of one step and the stream id of every row."""
        x = _cuda_f32(probs, "StreamingKeywordSpotter.step")
        B, T, V = x.shape
        if self._hd is None:
            if V < 1:
                raise ValueError("StreamingKeywordSpotter.step: the vocabulary is empty")
            self._create(V)
        if V != self.vocab:
            raise ValueError(f"StreamingKeywordSpotter.step: vocabulary {V}, the spotter has {self.vocab}")
        id_list = self._id_list(streams, B)
        ids = torch.tensor(id_list, dtype=torch.int32, device=self.device)
        if frames is None:
            fr = torch.full((B,), T, dtype=torch.int32, device=self.device)
        else:
            fr = torch.as_tensor(frames).to(device=self.device, dtype=torch.int32).reshape(-1)
            if fr.numel() != B or bool(((fr < 0) | (fr > T)).any()):
                raise ValueError(f"frames must be {B} counts in 0..{T}")
        res = torch.empty((B, 32), dtype=torch.uint8, device=self.device)
        if B:
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _capi.check(self._hd.lib.wekws_hip_ctc_kws_step(self._hd.h, x.data_ptr(), B, T, ids.data_ptr(), fr.data_ptr(),
                                                            res.data_ptr(), ctypes.c_void_p(stream)),
                        "wekws_hip_ctc_kws_step")
        return _results(res), id_list

    def _reset(self, streams, all_: int):
        if self._hd is None:
            return
        ids = self._ids(streams, len(streams) if streams is not None else self.num_streams)
        if ids.numel():
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _capi.check(self._hd.lib.wekws_hip_ctc_kws_reset(self._hd.h, ids.data_ptr(), ids.numel(), all_,
                                                             ctypes.c_void_p(stream)), "wekws_hip_ctc_kws_reset")

    def reset(self, streams=None):
        """KeyWordSpotter.reset() of the given streams (default all): the beam, activation and hit_score."""
        self._reset(streams, 0)

    def reset_all(self, streams=None):
        """KeyWordSpotter.reset_all(): reset() plus the frame offset and the last activation."""
        self._reset(streams, 1)

    def beams(self, stream: int):
        """The stream's cur_hyps: [(prefix, pb, pnb, [(token, frame, prob), ...]), ...] in beam order."""
        if self._hd is None:
            return [((), 1.0, 0.0, [])]
        if not 0 <= int(stream) < self.num_streams:
            raise ValueError(f"stream id {stream} outside 0..{self.num_streams - 1}")
        cap = self._cfg["prefix_capacity"]
        buf = torch.empty(self._hd.beam_bytes(cap), dtype=torch.uint8, device=self.device)
        s = torch.cuda.current_stream(self.device).cuda_stream
        _capi.check(self._hd.lib.wekws_hip_ctc_kws_read_beam(self._hd.h, int(stream), buf.data_ptr(), ctypes.c_void_p(s)),
                    "wekws_hip_ctc_kws_read_beam")
        return self._hd.decode_beam(buf.cpu().numpy(), cap)

    def status(self, stream: int) -> int:
        if self._hd is None:
            return 0
        out = ctypes.c_int32()
        s = torch.cuda.current_stream(self.device).cuda_stream
        _capi.check(self._hd.lib.wekws_hip_ctc_kws_status(self._hd.h, int(stream), ctypes.byref(out), ctypes.c_void_p(s)),
                    "wekws_hip_ctc_kws_status")
        return int(out.value)
