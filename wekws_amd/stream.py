"""``KeyWordSpotter.forward`` (wekws/bin/stream_kws_ctc.py:482-514) for many streams at once, PCM chunk in, detection out,
everything between on the device: the streaming front end (``accept_wave``: wekws_amd.frontend.StreamingFrontEnd), the
model with its carried cache, and the CTC prefix beam search with the keyword detection
(wekws_amd.ctc.StreamingKeywordSpotter).  No sample or feature crosses to the host except the chunk itself.

``BatchedThresholdSpotter`` is the same pipeline for max-pooling models (one sigmoid posterior per frame and keyword): the front
end, optionally delivering MFCC, the model, and the threshold scan of wekws_amd.det.StreamingThresholdSpotter."""
from __future__ import annotations

from typing import Dict, List

import torch

from wekws_amd import pack
from wekws_amd.ctc import StreamingKeywordSpotter
from wekws_amd.det import StreamingThresholdSpotter
from wekws_amd.frontend import StreamingFrontEnd, StreamingResampler, StreamingResamplerBank
from wekws_amd.model.kws_model import StreamCachePool


def _input_resampler(num_streams, input_rate, fe, device):
    """The resampler in front of the front end: none, a StreamingResampler for one input rate, a StreamingResamplerBank for a
    sequence of them (int16 out).  With one, the front end's ``max_chunk`` becomes the resampler's ``max_out``."""
    if input_rate is None:
        return None
    bank = isinstance(input_rate, (list, tuple))
    kind, rate = (StreamingResamplerBank, list(input_rate)) if bank else (StreamingResampler, int(input_rate))
    rs = kind(num_streams, rate, int(fe.get("sample_rate", 16000)), max_chunk=int(fe.get("max_chunk", 16000)), device=device)
    fe["max_chunk"] = rs.max_out(rs.max_chunk)
    return rs


def _set_input_rate(kws, streams, rate) -> None:
    if not isinstance(kws.resampler, StreamingResamplerBank):
        raise ValueError("set_input_rate needs a spotter built with a sequence of rates in input_sample_rate")
    kws.resampler.set_rate(streams, rate)       # (refuses a bad rate or stream before anything else is reset)
    kws.reset_all(streams)


class BatchedKeyWordSpotter:
    """``num_streams`` independent ``KeyWordSpotter`` objects behind one model.

        kws = BatchedKeyWordSpotter(model, {"hi_xiaowen": (12, 31, 7)}, 0.02, 4096, num_bins=80, window="povey",
                                    left=2, right=2, skip=3, max_chunk=4800)
        results = kws.forward(chunks)            # chunks: (B, nmax) int16 device tensor, or a list of bytes / int16 arrays

    ``model``: a ``wekws_amd`` KWSModel with a per-frame CTC head (``forward_softmax``).  The front-end settings are
    StreamingFrontEnd's (``num_bins``, ``window``, ``left``, ``right``, ``skip``, ``max_chunk``, ...), the others
    StreamingKeywordSpotter's (``min_frames``, ``max_frames``, ``interval_frames``, ``score_beam``, ``path_beam``,
    ``prefix_capacity``); ``downsampling`` is ``skip``.  ``input_sample_rate`` (e.g. 48000): the chunks arrive at that rate and
    pass a StreamingResampler (int16 out) to the front end's ``sample_rate`` first; ``max_chunk`` then counts INPUT samples.
    A sequence of rates (e.g. ``[16000, 48000, 8000]``) puts a StreamingResamplerBank there instead: every stream has its own
    input rate, the first one until ``kws.set_input_rate(streams, rate)`` says otherwise, and a step stays the same device calls.
    A member may be a ``(rate, encoding)`` pair (``wekws_amd.frontend.ENCODINGS``), e.g. ``[(8000, "mulaw"), 16000, (48000,
    "f32")]`` with ``kws.set_input_rate(streams, (8000, "mulaw"))``: those streams' chunks are G.711 bytes, unsigned 8-bit or
    float32, given as a list of ``bytes`` / arrays (each read in its stream's encoding) or as one (B, row_bytes) uint8 device
    tensor, and decoded inside the resampler's launch -- still the same device calls.

    Streams of different users may have different wake words: ``sid = kws.add_keywords({...}, threshold)`` registers a keyword
    set beside the constructor's, ``kws.set_keywords(sid, streams)`` gives it to streams (a new session for them),
    ``kws.drop_keywords(sid)`` frees it once no stream uses it.  A step is still the same three device calls."""

    _FE = ("num_bins", "window", "left", "right", "skip", "max_chunk", "sample_rate", "frame_length", "frame_shift", "num_ceps",
           "cepstral_lifter")

    def __init__(self, model, keywords, threshold: float, num_streams: int, **settings):
        fe = {k: settings.pop(k) for k in self._FE if k in settings}
        input_rate = settings.pop("input_sample_rate", None)
        self.model = model
        self.device = next(model.parameters()).device
        self.num_streams = int(num_streams)
        self.resampler = _input_resampler(self.num_streams, input_rate, fe, self.device)
        self.frontend = StreamingFrontEnd(self.num_streams, device=self.device, **fe)
        shift_ms = 1000.0 * self.frontend.cfg.fbank.frame_shift / self.frontend.cfg.fbank.sample_rate
        self.spotter = StreamingKeywordSpotter(self.num_streams, keywords, threshold, downsampling=self.frontend.skip,
                                               frame_shift_ms=shift_ms, device=self.device, **settings)
        # the carried cache of every stream, owned by the library; a fresh pool holds the empty-cache sentinel
        self.pool = StreamCachePool(model, self.num_streams, self.device)
        self.cache_axis = 1 if model._d["kind"] == "gru" else 0

    @property
    def cache(self) -> torch.Tensor:
        """The live cache of every stream, assembled in ``KWSModel.forward``'s geometry for ``num_streams`` rows (a copy)."""
        return torch.cat([self.pool.read(s) for s in range(self.num_streams)], dim=self.cache_axis)

    def forward(self, chunks, streams=None, samples=None, return_probs: bool = False):
        """One chunk per row; row b continues stream ``streams[b]`` (default 0 .. B-1).  Returns, per row,
        ``KeyWordSpotter.forward``'s dict -- ``{}`` for a row that was held or yielded no frame.  With ``return_probs`` also
        a list with each row's (frames, V) posteriors on the device (None for a row without frames) and the features the
        model was given.  Three device calls: the front end's push, the model step over the pool, the decoder's step (a
        fourth in front with ``input_sample_rate``: the resampler's push)."""
        if self.resampler is not None:
            chunks, samples = self.resampler.push(chunks, samples=samples, streams=streams)
        if torch.is_tensor(chunks):
            nmax = int(chunks.size(1)) if chunks.dim() == 2 else 0
        else:
            nmax = max([len(c) // 2 if isinstance(c, (bytes, bytearray, memoryview)) else len(c) for c in chunks] + [0])
        feats, frames = self.frontend.push(chunks, samples=samples, streams=streams, capacity=self.frontend.max_frames(nmax))
        B = len(frames)
        ids = list(range(B)) if streams is None else [int(s) for s in streams]
        if B == 0 or feats.size(1) == 0 or max(frames) <= 0:
            out: List[Dict] = [{} for _ in range(B)]
            return (out, [None] * B, [None] * B) if return_probs else out
        probs = self.model.forward_softmax_streams(feats, frames, ids, self.pool)
        out = self.spotter.step(probs, frames=[max(n, 0) for n in frames], streams=ids)
        if not return_probs:
            return out
        probs_out = [probs[b, :n] if n > 0 else None for b, n in enumerate(frames)]
        feats_out = [feats[b, :n] if n > 0 else None for b, n in enumerate(frames)]
        return out, probs_out, feats_out

    __call__ = forward

    def reset(self, streams=None) -> None:
        """KeyWordSpotter.reset(): the beam, activation and hit score of the streams (default all)."""
        self.spotter.reset(streams)

    def reset_all(self, streams=None) -> None:
        """KeyWordSpotter.reset_all(): reset() plus the frame offset and last activation, the front end's leftover samples,
        remembered frames and skip phase, the resampler's kept samples, and the streams' cache."""
        self.spotter.reset_all(streams)
        if self.resampler is not None:
            self.resampler.reset(streams)
        self.frontend.reset(streams)
        self.pool.reset(streams)

    def set_input_rate(self, streams, rate) -> None:
        """The streams (default all) arrive at ``rate`` from now on, one of the constructor's ``input_sample_rate`` sequence (Hz,
        or a ``(rate, encoding)`` pair).  A new session for them: the resampler's set_rate, and reset_all."""
        _set_input_rate(self, streams, rate)

    def add_keywords(self, keywords, threshold=None) -> int:
        """Register a keyword set beside the constructor's (StreamingKeywordSpotter.add_keywords); returns its id."""
        if self.spotter._hd is None:
            self.spotter._create(int(self.model.odim))
        return self.spotter.add_keywords(keywords, threshold)

    def set_keywords(self, set_id: int, streams=None) -> None:
        """``KeyWordSpotter.set_keywords`` for the given streams (default all): they use keyword set ``set_id`` from now on.  A stream that
        gets new keywords is a new session: the decoder's assign, and reset_all of the front end, the resampler and the cache."""
        self.spotter.assign(streams, set_id)
        if self.resampler is not None:
            self.resampler.reset(streams)
        self.frontend.reset(streams)
        self.pool.reset(streams)

    def drop_keywords(self, set_id: int) -> None:
        """Forget a keyword set no stream uses."""
        self.spotter.drop_keywords(set_id)


class BatchedThresholdSpotter:
    """``num_streams`` streams of a max-pooling model, PCM chunk in, threshold detections out.

        kws = BatchedThresholdSpotter(model, ["hi_xiaowen", "nihao_wenwen"], 0.5, 4096, num_bins=80, window="povey",
                                      num_ceps=80, max_chunk=4800)
        hits = kws.forward(chunks)               # per row: [{"keyword", "frame", "time", "score"}, ...]

    ``model``: a ``wekws_amd`` KWSModel whose head gives one posterior per frame and keyword (``odim == len(keywords)``).  The
    front-end settings are StreamingFrontEnd's (``num_ceps`` / ``cepstral_lifter`` for MFCC), ``input_sample_rate`` as for
    BatchedKeyWordSpotter, ``window_shift`` is StreamingThresholdSpotter's; ``threshold`` is one value or one per keyword."""

    _FE = BatchedKeyWordSpotter._FE
    cache = BatchedKeyWordSpotter.cache

    def __init__(self, model, keywords, threshold, num_streams: int, **settings):
        names = [str(k) for k in keywords]
        if model._d["head"] not in (pack.HEAD["linear"], pack.HEAD["identity"]) or model.odim != len(names):
            raise ValueError(f"BatchedThresholdSpotter needs a per-frame head with one output per keyword: the model gives "
                             f"{model.odim} for {len(names)} keywords")
        window_shift = settings.pop("window_shift", 50)
        fe = {k: settings.pop(k) for k in self._FE if k in settings}
        input_rate = settings.pop("input_sample_rate", None)
        if settings:
            raise TypeError(f"unknown settings {sorted(settings)}")
        self.model = model
        self.device = next(model.parameters()).device
        self.num_streams = int(num_streams)
        self.resampler = _input_resampler(self.num_streams, input_rate, fe, self.device)
        self.frontend = StreamingFrontEnd(self.num_streams, device=self.device, **fe)
        shift_ms = 1000.0 * self.frontend.cfg.fbank.frame_shift / self.frontend.cfg.fbank.sample_rate
        self.spotter = StreamingThresholdSpotter(self.num_streams, names, threshold, window_shift=window_shift,
                                                 downsampling=self.frontend.skip, frame_shift_ms=shift_ms, device=self.device)
        self.pool = StreamCachePool(model, self.num_streams, self.device)
        self.cache_axis = 1 if model._d["kind"] == "gru" else 0

    def forward(self, chunks, streams=None, samples=None, return_probs: bool = False):
        """One chunk per row; row b continues stream ``streams[b]`` (default 0 .. B-1).  Returns, per row, the list of its hits
        (empty for a row that was held or yielded no frame).  With ``return_probs`` also a list with each row's (frames, K)
        posteriors on the device (None for a row without frames) and the features the model was given.  Three device calls: the
        front end's push, the model step over the pool, the detector's step."""
        if self.resampler is not None:
            chunks, samples = self.resampler.push(chunks, samples=samples, streams=streams)
        if torch.is_tensor(chunks):
            nmax = int(chunks.size(1)) if chunks.dim() == 2 else 0
        else:
            nmax = max([len(c) // 2 if isinstance(c, (bytes, bytearray, memoryview)) else len(c) for c in chunks] + [0])
        feats, frames = self.frontend.push(chunks, samples=samples, streams=streams, capacity=self.frontend.max_frames(nmax))
        B = len(frames)
        ids = list(range(B)) if streams is None else [int(s) for s in streams]
        if B == 0 or feats.size(1) == 0 or max(frames) <= 0:
            out: List[List[Dict]] = [[] for _ in range(B)]
            return (out, [None] * B, [None] * B) if return_probs else out
        probs = self.model.forward_streams(feats, frames, ids, self.pool)
        out = self.spotter.step(probs, frames=[max(n, 0) for n in frames], streams=ids)
        if not return_probs:
            return out
        probs_out = [probs[b, :n] if n > 0 else None for b, n in enumerate(frames)]
        feats_out = [feats[b, :n] if n > 0 else None for b, n in enumerate(frames)]
        return out, probs_out, feats_out

    __call__ = forward

    def reset(self, streams=None) -> None:
        """The detector's state of the streams (default all): frame count, pending skip, running maximum."""
        self.spotter.reset(streams)

    def reset_all(self, streams=None) -> None:
        """reset() plus the front end's leftover samples, remembered frames and skip phase, the resampler's kept samples, and
        the streams' cache."""
        self.spotter.reset(streams)
        if self.resampler is not None:
            self.resampler.reset(streams)
        self.frontend.reset(streams)
        self.pool.reset(streams)

    def set_input_rate(self, streams, rate: int) -> None:
        """As BatchedKeyWordSpotter.set_input_rate."""
        _set_input_rate(self, streams, rate)
