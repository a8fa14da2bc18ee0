"""``KeyWordSpotter.forward`` (wekws/bin/stream_kws_ctc.py:482-514) for many streams at once, PCM chunk in, detection out,
everything between on the device: the streaming front end (``accept_wave``: wekws_amd.frontend.StreamingFrontEnd), the
model with its carried cache, and the CTC prefix beam search with the keyword detection
(wekws_amd.ctc.StreamingKeywordSpotter).  No sample or feature crosses to the host except the chunk itself."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from wekws_amd import pack
from wekws_amd.ctc import StreamingKeywordSpotter
from wekws_amd.frontend import StreamingFrontEnd


class BatchedKeyWordSpotter:
    """``num_streams`` independent ``KeyWordSpotter`` objects behind one model.

        kws = BatchedKeyWordSpotter(model, {"hi_xiaowen": (12, 31, 7)}, 0.02, 4096, num_bins=80, window="povey",
                                    left=2, right=2, skip=3, max_chunk=4800)
        results = kws.forward(chunks)            # chunks: (B, nmax) int16 device tensor, or a list of bytes / int16 arrays

    ``model``: a ``wekws_amd`` KWSModel with a per-frame CTC head (``forward_softmax``).  The front-end settings are
    StreamingFrontEnd's (``num_bins``, ``window``, ``left``, ``right``, ``skip``, ``max_chunk``, ...), the others
    StreamingKeywordSpotter's (``min_frames``, ``max_frames``, ``interval_frames``, ``score_beam``, ``path_beam``,
    ``prefix_capacity``); ``downsampling`` is ``skip``."""

    _FE = ("num_bins", "window", "left", "right", "skip", "max_chunk", "sample_rate", "frame_length", "frame_shift")

    def __init__(self, model, keywords, threshold: float, num_streams: int, **settings):
        fe = {k: settings.pop(k) for k in self._FE if k in settings}
        self.model = model
        self.device = next(model.parameters()).device
        self.num_streams = int(num_streams)
        self.frontend = StreamingFrontEnd(self.num_streams, device=self.device, **fe)
        shift_ms = 1000.0 * self.frontend.cfg.fbank.frame_shift / self.frontend.cfg.fbank.sample_rate
        self.spotter = StreamingKeywordSpotter(self.num_streams, keywords, threshold, downsampling=self.frontend.skip,
                                               frame_shift_ms=shift_ms, device=self.device, **settings)
        d = model._d
        # the carried cache of every stream; zeros are the empty-cache sentinel of a fresh stream
        self.cache = torch.zeros(pack.cache_shape(d, self.num_streams), dtype=torch.float32, device=self.device)
        self.cache_axis = 1 if d["kind"] == "gru" else 0

    def forward(self, chunks, streams=None, samples=None, return_probs: bool = False):
        """One chunk per row; row b continues stream ``streams[b]`` (default 0 .. B-1).  Returns, per row,
        ``KeyWordSpotter.forward``'s dict -- ``{}`` for a row that was held or yielded no frame.  With ``return_probs`` also
        a list with each row's (frames, V) posteriors on the device (None for a row without frames) and the features the
        model was given."""
        feats, frames = self.frontend.push(chunks, samples=samples, streams=streams)
        B = len(frames)
        ids = list(range(B)) if streams is None else [int(s) for s in streams]
        out: List[Dict] = [{} for _ in range(B)]
        probs_out: List[Optional[torch.Tensor]] = [None] * B
        feats_out: List[Optional[torch.Tensor]] = [None] * B
        # rows grouped by frame count: one model call and one decoder step per group
        groups: Dict[int, List[int]] = {}
        for b, n in enumerate(frames):
            if n > 0:
                groups.setdefault(n, []).append(b)
        for n, rows in sorted(groups.items()):
            ridx = torch.tensor(rows, dtype=torch.long, device=self.device)
            sidx = torch.tensor([ids[b] for b in rows], dtype=torch.long, device=self.device)
            x = feats.index_select(0, ridx)[:, :n].contiguous()
            cache = self.cache.index_select(self.cache_axis, sidx).contiguous()
            probs, cache = self.model.forward_softmax(x, cache)
            self.cache.index_copy_(self.cache_axis, sidx, cache)
            res = self.spotter.step(probs, streams=[ids[b] for b in rows])
            for j, b in enumerate(rows):
                out[b] = res[j]
                if return_probs:
                    probs_out[b], feats_out[b] = probs[j], x[j]
        return (out, probs_out, feats_out) if return_probs else out

    __call__ = forward

    def reset(self, streams=None) -> None:
        """KeyWordSpotter.reset(): the beam, activation and hit score of the streams (default all)."""
        self.spotter.reset(streams)

    def reset_all(self, streams=None) -> None:
        """KeyWordSpotter.reset_all(): reset() plus the frame offset and last activation, the front end's leftover samples,
        remembered frames and skip phase, and the streams' cache."""
        self.spotter.reset_all(streams)
        self.frontend.reset(streams)
        if streams is None:
            self.cache.zero_()
        else:
            sidx = torch.tensor([int(s) for s in streams], dtype=torch.long, device=self.device)
            self.cache.index_fill_(self.cache_axis, sidx, 0.0)
