"""Device side of the DET evaluation: the score reductions of wekws/bin/compute_det.py:79-106 on the per-frame
posteriors that wekws/bin/score.py:128-137 would write to a text file -- per-utterance maxima (false rejects) and
sliding-window alarm counts (false alarms) -- so that an evaluation loop keeps the (B, T, K) score matrix on the GPU.
Comparisons only: bit-exact with the reference's Python on the same float32 scores.

StreamingThresholdSpotter carries the alarm scan across chunks for many streams at once (wekws_hip_threshold_kws_*): the
detector of a max-pooling model behind KWSModel.forward_streams."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from wekws_amd import _capi


def det_thresholds(step: float = 0.01) -> np.ndarray:
    """The thresholds compute_det.py:78-79,105 visits: `threshold = 0.0; while threshold <= 1.0: ...; threshold += step`
    (float64 accumulation, so the list is exactly the reference's)."""
    out, th = [], 0.0
    while th <= 1.0:
        out.append(th)
        th += step
    return np.asarray(out, np.float64)


def _check(scores: torch.Tensor, lengths: Optional[torch.Tensor]):
    if not scores.is_cuda or scores.dtype != torch.float32 or scores.dim() != 3:
        raise ValueError("scores must be a (B, T, K) float32 tensor on a ROCm device (no CPU fallback)")
    s = scores.contiguous()
    ln = None
    if lengths is not None:
        ln = lengths.to(device=s.device, dtype=torch.int32).contiguous()
        if ln.numel() != s.size(0):
            raise ValueError("lengths must have one entry per utterance")
    return s, ln


def max_pool_scores(scores: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(B, T, K) posteriors -> (max (B, K) float32, first arg-max frame (B, K) int64): `max(score_list)` of
    compute_det.py:84 for every utterance and keyword, over the first lengths[b] frames (score.py:131)."""
    s, ln = _check(scores, lengths)
    B, T, K = (int(v) for v in s.shape)
    mx = torch.empty((B, K), dtype=torch.float32, device=s.device)
    am = torch.empty((B, K), dtype=torch.int32, device=s.device)
    if B and T and K:
        stream = torch.cuda.current_stream(s.device).cuda_stream
        _capi.check(_capi.load().wekws_hip_score_maxpool(s.data_ptr(), B, T, K, ln.data_ptr() if ln is not None else None,
                                                         mx.data_ptr(), am.data_ptr(), ctypes.c_void_p(stream)),
                    "wekws_hip_score_maxpool")
    return mx, am.to(torch.int64)


def round_like_score_file(values: np.ndarray) -> np.ndarray:
    """float64 values as compute_det.py sees scores after score.py:134-135 wrote them as '{:.6f}' text."""
    return np.asarray([float("{:.6f}".format(v)) for v in np.asarray(values, np.float64).ravel()],
                      np.float64).reshape(np.shape(values))


def false_alarm_counts(scores: torch.Tensor, keyword: int, thresholds: Sequence[float], window_shift: int = 50,
                       lengths: Optional[torch.Tensor] = None, text_format: bool = False) -> torch.Tensor:
    """(B, T, K) posteriors -> (B, n_thr) int32 alarm counts of column `keyword`: the scan of compute_det.py:88-96.
    text_format: compare the scores rounded to six decimals, i.e. as the reference's score text file carries them."""
    s, ln = _check(scores, lengths)
    B, T, K = (int(v) for v in s.shape)
    th = torch.from_numpy(np.ascontiguousarray(thresholds, np.float64)).to(s.device)
    out = torch.empty((B, th.numel()), dtype=torch.int32, device=s.device)
    if B and T and K:
        stream = torch.cuda.current_stream(s.device).cuda_stream
        lib = _capi.load()
        fn = lib.wekws_hip_det_false_alarms_text if text_format else lib.wekws_hip_det_false_alarms
        _capi.check(fn(s.data_ptr(), B, T, K, int(keyword), ln.data_ptr() if ln is not None else None, th.data_ptr(),
                       int(th.numel()), int(window_shift), out.data_ptr(), ctypes.c_void_p(stream)),
                    "wekws_hip_det_false_alarms")
    return out


def det_stats(scores: torch.Tensor, lengths: Optional[torch.Tensor], is_keyword: Sequence[bool], keyword: int,
              filler_duration: float, step: float = 0.01, window_shift: int = 50,
              text_format: bool = False) -> List[Tuple[float, float, float]]:
    """The rows compute_det.py:97-104 writes to its stats file -- (threshold, false alarms per hour, false reject rate)
    -- for one keyword column of a scored batch: `is_keyword[b]` says whether utterance b's transcript is the keyword
    (compute_det.py:45-50).  Only the (B,) maxima and the (B, n_thr) counts leave the device.
    text_format=True reproduces the stats file of the reference's score.py -> compute_det.py chain bit for bit: there the
    scores pass through '{:.6f}' text (score.py:134-135) before they are compared."""
    kw = np.asarray(list(is_keyword), bool)
    # the reference assigns the two rates only under `if len(keyword_table) != 0` / `if filler_duration != 0` (compute_det.py:97-101)
    # and then formats them: an evaluation set without a keyword utterance, or without filler audio, dies there with NameError
    if filler_duration == 0:
        raise NameError("name 'false_alarm_per_hour' is not defined")
    if not kw.any():
        raise NameError("name 'false_reject_rate' is not defined")
    if lengths is not None and bool((lengths.cpu().numpy()[kw] <= 0).any()):
        raise ValueError("max() arg is an empty sequence")       # compute_det.py:84 `max(score_list)` of a keyword utterance without frames
    th = det_thresholds(step)
    mx, _ = max_pool_scores(scores, lengths)
    alarms = false_alarm_counts(scores, keyword, th, window_shift, lengths, text_format=text_format).cpu().numpy()
    mk = mx[:, keyword].cpu().numpy().astype(np.float64)[kw]
    if text_format:
        mk = round_like_score_file(mk)                       # max and a monotonic rounding commute
    rows = []
    false_reject_rate = false_alarm_per_hour = 0.0
    for j, t in enumerate(th):
        num_false_reject = int((mk < t).sum())
        num_false_alarm = int(alarms[~kw, j].sum())
        if kw.any():
            false_reject_rate = num_false_reject / int(kw.sum())
        num_false_alarm = max(num_false_alarm, 1e-6)
        if filler_duration != 0:
            false_alarm_per_hour = num_false_alarm / (filler_duration / 3600.0)
        rows.append((float(t), float(false_alarm_per_hour), float(false_reject_rate)))
    return rows


class StreamingThresholdSpotter:
    """The alarm scan of compute_det.py:89-96 carried across chunks, for ``num_streams`` streams on one device: per stream and
    keyword (each keyword on its own), a frame fires iff it is not inside the ``window_shift`` frames behind the last hit and
    its score is >= the keyword's threshold.  For any split of a score sequence into chunks the hits are those of one scan.

        spot = StreamingThresholdSpotter(4096, ["hi_xiaowen", "nihao_wenwen"], 0.5)
        hits = spot.step(probs, frames, streams)    # probs (B, T, K) sigmoid posteriors on the device

    ``threshold``: one value, or one per keyword.  A hit's ``frame`` counts the frames the stream was given since its reset;
    ``time`` = frame * downsampling * frame_shift_ms / 1000 seconds."""

    def __init__(self, num_streams: int, keywords, threshold, window_shift: int = 50, downsampling: int = 1,
                 frame_shift_ms: float = 10, device=None):
        self.names = [str(k) for k in keywords]
        K = len(self.names)
        th = np.asarray(threshold, np.float64).reshape(-1)
        if th.size == 1:
            th = np.full(K, float(th[0]), np.float64)
        if K < 1 or th.size != K:
            raise ValueError(f"{th.size} thresholds for {K} keywords (need one, or one per keyword, and a keyword)")
        if int(window_shift) < 1 or int(num_streams) < 1:
            raise ValueError("window_shift and num_streams must be >= 1")
        self.thresholds = np.ascontiguousarray(th)
        self.num_streams, self.window_shift = int(num_streams), int(window_shift)
        self.resolution = int(downsampling) * frame_shift_ms / 1000
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError("StreamingThresholdSpotter runs on the MI355X HIP path only (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = _capi.load()
        self._ptr = ctypes.c_void_p()
        _capi.check(self._lib.wekws_hip_threshold_kws_create(
            K, self.thresholds.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), self.window_shift, self.num_streams,
            self.device.index, ctypes.byref(self._ptr)), "wekws_hip_threshold_kws_create")

    def __del__(self):
        try:
            if self._ptr:
                self._lib.wekws_hip_threshold_kws_destroy(self._ptr)
                self._ptr = ctypes.c_void_p()
        except Exception:
            pass

    def _ids(self, streams, n: int) -> torch.Tensor:
        if streams is None and n <= self.num_streams:              # 0 .. n-1: made on the device, nothing to check or upload
            return torch.arange(n, dtype=torch.int32, device=self.device)
        ids = list(range(n)) if streams is None else [int(s) for s in (streams.tolist() if hasattr(streams, "tolist") else streams)]
        if len(ids) != n:
            raise ValueError(f"{len(ids)} stream ids for {n} rows")
        if len(set(ids)) != len(ids) or any(s < 0 or s >= self.num_streams for s in ids):
            raise ValueError(f"stream ids must be distinct and in 0..{self.num_streams - 1}")
        return torch.tensor(ids, dtype=torch.int32, device=self.device)

    def step_records(self, probs: torch.Tensor, frames=None, streams=None):
        """One chunk per row, no synchronise with device ``frames``: returns the device tensors ``(hit_frames (B, K, D) int32,
        ascending, -1 fill; hit_scores (B, K, D); best (B, K); best_frame (B, K) int32; status (B) int32)``, D =
        ceil(T / window_shift).  ``frames`` given as host values is checked here; a device tensor is checked by the kernel
        alone, which skips a bad row and says so in ``status``."""
        if not torch.is_tensor(probs) or not probs.is_cuda or probs.dtype != torch.float32 or probs.dim() != 3:
            raise ValueError("probs must be a (B, T, K) float32 tensor on a ROCm device (no CPU fallback)")
        x = probs.contiguous()
        B, T, K = (int(v) for v in x.shape)
        if K != len(self.names):
            raise ValueError(f"probs carry {K} keywords, the spotter has {len(self.names)}")
        ids = self._ids(streams, B)
        fr = None
        if frames is not None:
            if torch.is_tensor(frames) and frames.is_cuda:
                fr = frames.to(dtype=torch.int32).reshape(-1).contiguous()
                if fr.numel() != B:
                    raise ValueError(f"frames must be {B} counts in 0..{T}")
            else:
                host = np.asarray(frames.tolist() if hasattr(frames, "tolist") else list(frames), np.int64).reshape(-1)
                if host.size != B or bool(((host < 0) | (host > T)).any()):
                    raise ValueError(f"frames must be {B} counts in 0..{T}")
                fr = torch.from_numpy(host.astype(np.int32)).to(self.device)
        D = int(self._lib.wekws_hip_threshold_kws_max_hits(self._ptr, T))
        dev = x.device
        hf = torch.empty((B, K, D), dtype=torch.int32, device=dev)
        hs = torch.empty((B, K, D), dtype=torch.float32, device=dev)
        best = torch.empty((B, K), dtype=torch.float32, device=dev)
        bf = torch.empty((B, K), dtype=torch.int32, device=dev)
        status = torch.zeros((B,), dtype=torch.int32, device=dev)
        if B:
            stream = torch.cuda.current_stream(dev).cuda_stream
            _capi.check(self._lib.wekws_hip_threshold_kws_step(
                self._ptr, x.data_ptr() if T else None, B, T, ids.data_ptr(), fr.data_ptr() if fr is not None else None,
                hf.data_ptr() if D else None, hs.data_ptr() if D else None, best.data_ptr(), bf.data_ptr(), status.data_ptr(),
                ctypes.c_void_p(stream)), "wekws_hip_threshold_kws_step")
        return hf, hs, best, bf, status

    def step(self, probs: torch.Tensor, frames=None, streams=None) -> List[List[Dict]]:
        """Per row the hits of its chunk, ordered by frame and then keyword:
        ``[{"keyword": name, "frame": frames since reset, "time": seconds, "score": float}, ...]``."""
        hf, hs, _, _, status = self.step_records(probs, frames, streams)
        hf, hs, status = hf.cpu().numpy(), hs.cpu().numpy(), status.cpu().numpy()
        if status.any():
            raise ValueError(f"StreamingThresholdSpotter.step: rows {np.nonzero(status)[0].tolist()} were skipped "
                             f"(status {status[status != 0].tolist()}: 1 = frame count, 2 = stream id, 3 = frame index range)")
        out = []
        for b in range(hf.shape[0]):
            ks, ds = np.nonzero(hf[b] >= 0)
            hits = sorted((int(hf[b, k, d]), int(k), float(hs[b, k, d])) for k, d in zip(ks, ds))
            out.append([{"keyword": self.names[k], "frame": a, "time": a * self.resolution, "score": v} for a, k, v in hits])
        return out

    def reset(self, streams=None) -> None:
        """The streams (default all) start over: frame 0, no skip pending, no maximum."""
        ids = self._ids(streams, len(streams) if streams is not None else self.num_streams)
        if ids.numel():
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _capi.check(self._lib.wekws_hip_threshold_kws_reset(self._ptr, ids.data_ptr(), ids.numel(), ctypes.c_void_p(stream)),
                        "wekws_hip_threshold_kws_reset")

    def state(self, stream: int, keyword: int) -> Dict:
        """``{"seen", "resume", "best_frame", "best"}`` of one (stream, keyword); synchronises."""
        if not 0 <= int(stream) < self.num_streams or not 0 <= int(keyword) < len(self.names):
            raise ValueError(f"stream {stream} / keyword {keyword} out of range")
        slot = _capi.ThresholdKwsSlot()
        s = torch.cuda.current_stream(self.device).cuda_stream
        _capi.check(self._lib.wekws_hip_threshold_kws_state(self._ptr, int(stream), int(keyword), ctypes.byref(slot),
                                                            ctypes.c_void_p(s)), "wekws_hip_threshold_kws_state")
        return {"seen": int(slot.seen), "resume": int(slot.resume), "best_frame": int(slot.best_frame), "best": float(slot.best)}

    def best(self, stream: int) -> Tuple[List[float], List[int]]:
        """The running maximum of the stream's keywords since its reset and the first frame that attained it
        (-inf / -1 before any frame)."""
        st = [self.state(stream, k) for k in range(len(self.names))]
        return [s["best"] for s in st], [s["best_frame"] for s in st]
