"""Batched on-device front-end: log-mel filterbank (MI355X replacement for ``wenet::Fbank::Compute``,
runtime/core/frontend/fbank.h:138-198, behind ``FeaturePipeline::AcceptWaveform``'s framing rule,
runtime/core/frontend/feature_pipeline.cc:30-47) and the context-expansion / frame-skip step of the data pipeline
(wekws/dataset/init_dataset.py:24-68), and in front of both the `resample` step (wekws/dataset/processor.py:83-103).  Thin
host wrappers over the C ABI (wekws_hip_fbank_*, wekws_hip_splice, wekws_hip_resample_*, wekws_hip_resample_bank_* with the wire encodings of its members); no CPU
fallback."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from wekws_amd import _capi

WINDOWS = dict(hamming=0, povey=1)


class Fbank:
    """feats = Fbank(num_bins=40)(pcm)  with pcm (B, nsamp) float32 in int16 scale on a ROCm device
    (the runtime never divides by 32768: runtime/core/frontend/wav.h:98-102) -> (B, frames, num_bins).

    ``dither`` > 0: the training recipes' ``dither: 1.0`` (wekws/dataset/processor.py:134-203) -- ``frame[i] += dither * N(0, 1)``
    after framing, before DC removal, drawn inside the kernel.  The draw at (``seed``, row id, frame, sample) is a pure function
    of those four numbers; row b of a call has row id ``first_row + b``, by default the object's own row counter, which advances
    by B per call (``reset_rows`` sets it): a data set cut into batches in any way gets the same noise per utterance.

        fb = Fbank(80, window="povey", dither=1.0, seed=777)
        feats = fb(pcm)                         # rows 0 .. B-1; the next call continues at B"""

    def __init__(self, num_bins: int = 40, sample_rate: int = 16000, frame_length: Optional[int] = None,
                 frame_shift: Optional[int] = None, window: str = "hamming", device="cuda", dither: float = 0.0, seed: int = 0):
        # FeaturePipelineConfig: 25 ms window, 10 ms shift (feature_pipeline.h:34-39)
        self.num_bins = num_bins
        self.sample_rate = sample_rate
        self.frame_length = frame_length if frame_length is not None else sample_rate // 1000 * 25
        self.frame_shift = frame_shift if frame_shift is not None else sample_rate // 1000 * 10
        if window not in WINDOWS:
            raise ValueError(f"window must be one of {sorted(WINDOWS)}")
        self.dither, self.seed, self.next_row = float(dither), int(seed), 0
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError("seed must be an unsigned 64-bit integer")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("wekws_amd.frontend.Fbank runs on the MI355X HIP path only (no CPU fallback)")
        lib = _capi.load()
        cfg = _capi.FbankCfg()
        cfg.num_bins, cfg.sample_rate = num_bins, sample_rate
        cfg.frame_length, cfg.frame_shift, cfg.window = self.frame_length, self.frame_shift, WINDOWS[window]
        self._lib = lib
        self._ptr = ctypes.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _capi.check(lib.wekws_hip_fbank_create(ctypes.byref(cfg), idx, ctypes.byref(self._ptr)), "wekws_hip_fbank_create")

    def __del__(self):
        try:
            if self._ptr:
                self._lib.wekws_hip_fbank_destroy(self._ptr)
                self._ptr = ctypes.c_void_p()
        except Exception:
            pass

    def num_frames(self, nsamp: int) -> int:
        return int(self._lib.wekws_hip_fbank_num_frames(self._ptr, int(nsamp)))

    def reset_rows(self, n: int = 0) -> None:
        """The row id the next call without ``first_row`` starts at."""
        self.next_row = int(n)

    def __call__(self, pcm: torch.Tensor, first_row: Optional[int] = None) -> torch.Tensor:
        """(B, nsamp) PCM on a ROCm device -> (B, frames, num_bins) log-mel.  float32 in int16 scale (wav.h:98-102), or
        int16 as FeaturePipeline::AcceptWaveform(std::vector<int16_t>) receives it (feature_pipeline.cc:49-55): widened
        in the kernel's registers -- 2 bytes per sample over PCIe and HBM, the same features bit for bit.
        ``first_row``: the row id of row 0 for the dither's draws (default: the object's counter, advanced by B)."""
        if pcm.dim() != 2 or not pcm.is_cuda or pcm.dtype not in (torch.float32, torch.int16):
            raise ValueError("pcm must be a (B, nsamp) float32 or int16 tensor on a ROCm device")
        pcm = pcm.contiguous()
        B, n = int(pcm.size(0)), int(pcm.size(1))
        nf = self.num_frames(n)
        feats = torch.empty((B, nf, self.num_bins), dtype=torch.float32, device=pcm.device)
        row0 = self.next_row if first_row is None else int(first_row)
        if B and nf:
            stream = torch.cuda.current_stream(pcm.device).cuda_stream
            if self.dither == 0.0:
                fn = self._lib.wekws_hip_fbank_compute if pcm.dtype == torch.float32 else self._lib.wekws_hip_fbank_compute_i16
                _capi.check(fn(self._ptr, pcm.data_ptr(), B, n, feats.data_ptr(), ctypes.c_void_p(stream)), "wekws_hip_fbank_compute")
            else:
                fn = self._lib.wekws_hip_fbank_compute_dither if pcm.dtype == torch.float32 else \
                    self._lib.wekws_hip_fbank_compute_dither_i16
                _capi.check(fn(self._ptr, pcm.data_ptr(), B, n, feats.data_ptr(), self.dither, self.seed, row0,
                               ctypes.c_void_p(stream)), "wekws_hip_fbank_compute_dither")
        if first_row is None:
            self.next_row = row0 + B
        return feats

    def leftover(self, nsamp: int) -> Tuple[int, int]:
        """(frames, first sample to keep) for a streaming caller: the reference keeps
        samples[frame_shift * frames:] for the next push (feature_pipeline.cc:41-44)."""
        nf = self.num_frames(nsamp)
        return nf, self.frame_shift * nf


def splice_skip(feats: torch.Tensor, left: int = 0, right: int = 0, skip: int = 1,
                feats_lengths: Optional[torch.Tensor] = None):
    """context_expansion(left, right) followed by frame_skip(skip) (wekws/dataset/init_dataset.py:24-68) as ONE
    gather on the device: (B, T, F) -> (B, ceil((T - right) / skip), (left + right + 1) * F).
    With ``feats_lengths`` also returns the reference's updated lengths (:51 then :64-65).
    Degenerate lengths behave like the reference: ``left >= T`` raises IndexError (its left-margin loop), ``T < right``
    returns the ``2 T - right`` wrapped frames its negative slice keeps (include/wekws_hip.h)."""
    if feats.dim() != 3 or not feats.is_cuda or feats.dtype != torch.float32:
        raise ValueError("feats must be a (B, T, F) float32 tensor on a ROCm device (no CPU fallback)")
    lib = _capi.load()
    feats = feats.contiguous()
    B, T, F = (int(v) for v in feats.shape)
    if left >= 1 and left >= T:                 # init_dataset.py:45-48 reads feats_ctx[:, left]: the reference's own error
        raise IndexError(f"index {int(left)} is out of bounds for dimension 1 with size {T}")
    To = int(lib.wekws_hip_splice_frames(T, int(right), int(skip)))
    out = torch.empty((B, To, (left + right + 1) * F), dtype=torch.float32, device=feats.device)
    if B and To:
        stream = torch.cuda.current_stream(feats.device).cuda_stream
        _capi.check(lib.wekws_hip_splice(feats.data_ptr(), B, T, F, int(left), int(right), int(skip), out.data_ptr(),
                                         ctypes.c_void_p(stream)), "wekws_hip_splice")
    if feats_lengths is None:
        return out
    lens = torch.ceil((feats_lengths - right) / skip).to(dtype=torch.int16)
    return out, lens


def context_expansion(feats: torch.Tensor, left: int = 1, right: int = 1) -> torch.Tensor:
    """wekws/dataset/init_dataset.py:24-52 on a (B, T, F) device batch."""
    return splice_skip(feats, left, right, 1)


def frame_skip(feats: torch.Tensor, skip_rate: int = 1) -> torch.Tensor:
    """wekws/dataset/init_dataset.py:54-68 on a (B, T, F) device batch."""
    return splice_skip(feats, 0, 0, skip_rate)


def dither_noise(seed: int, first_row: int, B: int, nframes: int, frame_length: int, device="cuda") -> torch.Tensor:
    """The (B, nframes, frame_length) unit-variance normal field that ``Fbank(dither=d, seed=seed)`` scales by d and adds to the
    frames of rows ``first_row .. first_row + B - 1`` (wekws_hip_dither_noise; the definition: csrc/philox.hip.h)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("wekws_amd.frontend.dither_noise runs on the MI355X HIP path only (no CPU fallback)")
    lib = _capi.load()
    with torch.cuda.device(device):
        out = torch.empty((int(B), int(nframes), int(frame_length)), dtype=torch.float32, device=device)
        stream = torch.cuda.current_stream(device).cuda_stream
        _capi.check(lib.wekws_hip_dither_noise(int(seed), int(first_row), int(B), int(nframes), int(frame_length),
                                               out.data_ptr() if out.numel() else None, ctypes.c_void_p(stream)), "wekws_hip_dither_noise")
    return out


def dct_lifter(logmel: torch.Tensor, num_ceps: int, cepstral_lifter: float = 22.0) -> torch.Tensor:
    """The MFCC tail of torchaudio.compliance.kaldi.mfcc (DCT-II 'ortho' with Kaldi's first column, first ``num_ceps``
    cepstra, cepstral lifter) on (..., num_mel_bins) log-mel rows -> (..., num_ceps); wekws_hip_dct_lifter."""
    if not logmel.is_cuda or logmel.dtype != torch.float32:
        raise ValueError("logmel must be a float32 tensor on a ROCm device (no CPU fallback)")
    lib = _capi.load()
    logmel = logmel.contiguous()
    nb = int(logmel.shape[-1])
    rows = logmel.numel() // nb if nb else 0
    out = torch.empty(tuple(logmel.shape[:-1]) + (int(num_ceps),), dtype=torch.float32, device=logmel.device)
    stream = torch.cuda.current_stream(logmel.device).cuda_stream
    _capi.check(lib.wekws_hip_dct_lifter(logmel.data_ptr(), rows, nb, int(num_ceps), float(cepstral_lifter),
                                         out.data_ptr(), ctypes.c_void_p(stream)), "wekws_hip_dct_lifter")
    return out


class Mfcc:
    """``kaldi.mfcc(waveform * (1 << 15), num_ceps, num_mel_bins, frame_length, frame_shift, energy_floor=0.0,
    sample_frequency)`` of the reference's MDTC recipes (wekws/dataset/processor.py:134-169) on the device: Povey-window
    fbank (wekws_hip_fbank_*) followed by the DCT / lifter kernel.  ``pcm`` is (B, nsamp) float32 already in int16 scale.
    ``dither`` / ``seed`` / ``first_row`` / ``reset_rows``: as for ``Fbank`` (the recipes' ``mfcc_conf`` sets ``dither: 1.0``).
    Parity with torchaudio is unpinned (see oracle/kaldi_feats_oracle.py)."""

    def __init__(self, num_ceps: int = 80, num_mel_bins: int = 80, sample_rate: int = 16000, cepstral_lifter: float = 22.0,
                 device="cuda", dither: float = 0.0, seed: int = 0):
        if not 0 < num_ceps <= num_mel_bins:
            raise ValueError("need 0 < num_ceps <= num_mel_bins")
        self.num_ceps, self.cepstral_lifter = int(num_ceps), float(cepstral_lifter)
        self.fbank = Fbank(num_mel_bins, sample_rate, window="povey", device=device, dither=dither, seed=seed)

    def reset_rows(self, n: int = 0) -> None:
        self.fbank.reset_rows(n)

    def __call__(self, pcm: torch.Tensor, first_row: Optional[int] = None) -> torch.Tensor:
        return dct_lifter(self.fbank(pcm, first_row), self.num_ceps, self.cepstral_lifter)


class StreamingFrontEnd:
    """``KeyWordSpotter.accept_wave`` (wekws/bin/stream_kws_ctc.py:335-398) for ``num_streams`` streams at once, on the
    device: leftover samples, Kaldi fbank of (leftover + chunk), the remembered frames of the context expansion and the
    frame-skip phase are carried per stream by the library (wekws_hip_stream_frontend_*); a push is two launches.

        fe = StreamingFrontEnd(4096, num_bins=80, window="povey", left=2, right=2, skip=3, max_chunk=4800)
        feats, frames = fe.push(pcm)            # pcm (B, nmax) int16 on the device: row b continues stream b

    Context is off (left = right = 0) or ``left == right >= 1``; anything else is refused (the streaming reference is
    coherent only there).  int16 input only, as the reference receives it.

    ``num_ceps``: None for log-mel rows; else every frame leaves the fbank kernel as ``num_ceps`` cepstra (``Mfcc``'s DCT and
    ``cepstral_lifter``, applied by the wave that finished the frame: still two launches), bit for bit
    ``dct_lifter(Fbank(...)(whole signal), num_ceps, cepstral_lifter)``; ``feat_dim = num_ceps * (left + right + 1)``.  The
    reference's MDTC recipes: ``num_bins=80, window="povey", num_ceps=80``."""

    def __init__(self, num_streams: int, num_bins: int = 40, window: str = "hamming", left: int = 0, right: int = 0,
                 skip: int = 1, max_chunk: int = 16000, sample_rate: int = 16000, frame_length: Optional[int] = None,
                 frame_shift: Optional[int] = None, device="cuda", num_ceps: Optional[int] = None, cepstral_lifter: float = 22.0):
        if window not in WINDOWS:
            raise ValueError(f"window must be one of {sorted(WINDOWS)}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("wekws_amd.frontend.StreamingFrontEnd runs on the MI355X HIP path only (no CPU fallback)")
        self.num_streams, self.num_bins, self.max_chunk = int(num_streams), int(num_bins), int(max_chunk)
        self.left, self.right, self.skip = int(left), int(right), int(skip)
        self.num_ceps = None if num_ceps is None else int(num_ceps)
        self.cepstral_lifter = float(cepstral_lifter)
        self.frame_dim = self.num_bins if self.num_ceps is None else self.num_ceps     # floats of one frame
        self.feat_dim = self.frame_dim * (self.left + self.right + 1)
        cfg = _capi.StreamFrontendCfg()
        cfg.fbank.num_bins, cfg.fbank.sample_rate = self.num_bins, int(sample_rate)
        cfg.fbank.frame_length = int(frame_length) if frame_length is not None else sample_rate // 1000 * 25
        cfg.fbank.frame_shift = int(frame_shift) if frame_shift is not None else sample_rate // 1000 * 10
        cfg.fbank.window = WINDOWS[window]
        cfg.left, cfg.right, cfg.skip = self.left, self.right, self.skip
        cfg.max_streams, cfg.max_chunk = self.num_streams, self.max_chunk
        cfg.device = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", cfg.device)
        self.cfg = cfg
        self._lib = _capi.load()
        self._ptr = ctypes.c_void_p()
        if self.num_ceps is None:
            _capi.check(self._lib.wekws_hip_stream_frontend_create(ctypes.byref(cfg), ctypes.byref(self._ptr)),
                        "wekws_hip_stream_frontend_create")
        else:
            _capi.check(self._lib.wekws_hip_stream_frontend_create_mfcc(ctypes.byref(cfg), self.num_ceps, self.cepstral_lifter,
                                                                        ctypes.byref(self._ptr)),
                        "wekws_hip_stream_frontend_create_mfcc")

    def __del__(self):
        try:
            if self._ptr:
                self._lib.wekws_hip_stream_frontend_destroy(self._ptr)
                self._ptr = ctypes.c_void_p()
        except Exception:
            pass

    def max_frames(self, nmax: int) -> int:
        """A row capacity that always suffices for chunks of up to ``nmax`` samples."""
        return int(self._lib.wekws_hip_stream_frontend_max_frames(self._ptr, int(nmax)))

    def push(self, pcm, samples=None, streams=None, capacity: Optional[int] = None, out: Optional[torch.Tensor] = None):
        """``pcm``: a (B, nmax) int16 device tensor, or a list of ``bytes`` / int16 arrays (uploaded as ONE padded tensor);
        ``samples``: the valid samples per row (default: all, or each list entry's own length); ``streams``: the stream of
        each row (default 0 .. B-1).  Returns ``(feats, frames)``: feats (B, max(frames, 0), D) float32 on the device, zero
        past each row's count; frames a host list, -1 = held (the reference's None), 0 = its empty result.
        ``capacity``: rows to allocate per stream (default: ``max_frames(nmax)``), for a caller that wants one shape.
        ``out``: a (B, capacity, D) float32 device tensor to write into instead (rows past a count keep what they held)."""
        if not torch.is_tensor(pcm):
            arrs = [np.frombuffer(c, dtype="<i2") if isinstance(c, (bytes, bytearray, memoryview)) else np.asarray(c) for c in pcm]
            if any(a.dtype != np.int16 or a.ndim != 1 for a in arrs):
                raise ValueError("chunks must be bytes or 1-d int16 arrays")
            if samples is None:
                samples = [int(a.size) for a in arrs]
            host = np.zeros((len(arrs), max([int(a.size) for a in arrs] + [0])), dtype=np.int16)
            for i, a in enumerate(arrs):
                host[i, :a.size] = a
            pcm = torch.from_numpy(host).to(self.device)
        if pcm.dim() != 2 or not pcm.is_cuda or pcm.dtype != torch.int16:
            raise ValueError("pcm must be a (B, nmax) int16 tensor on a ROCm device")
        pcm = pcm.contiguous()
        B, nmax = int(pcm.size(0)), int(pcm.size(1))
        # host arguments as int32 arrays (thousands of rows: no per-row Python objects on the way in)
        ids = np.arange(B, dtype=np.int32) if streams is None else np.asarray([int(s) for s in streams], dtype=np.int64)
        ns = np.full(B, nmax, dtype=np.int32) if samples is None else np.asarray([int(n) for n in samples], dtype=np.int64)
        if ids.shape != (B,) or ns.shape != (B,):
            raise ValueError("streams / samples must have one entry per row of pcm")
        lim = np.iinfo(np.int32)
        ids = np.ascontiguousarray(np.clip(ids, lim.min, lim.max), dtype=np.int32)     # (out of range stays out of range: EINVAL)
        ns = np.ascontiguousarray(np.clip(ns, lim.min, lim.max), dtype=np.int32)
        if out is not None:
            if out.dim() != 3 or out.size(0) != B or out.size(2) != self.feat_dim or out.dtype != torch.float32 or \
                    out.device != pcm.device or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous ({B}, capacity, {self.feat_dim}) float32 tensor on the device of pcm")
            cap, feats, capacity = int(out.size(1)), out, int(out.size(1))
        else:
            cap = self.max_frames(nmax) if capacity is None else int(capacity)
            feats = torch.zeros((B, cap, self.feat_dim), dtype=torch.float32, device=pcm.device)
        got = np.zeros(max(B, 1), dtype=np.int32)
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        _capi.check(self._lib.wekws_hip_stream_frontend_push(
            self._ptr, pcm.data_ptr() if nmax else None, B, nmax, ids.ctypes.data if B else None, ns.ctypes.data if B else None,
            feats.data_ptr() if cap else None, cap, got.ctypes.data, ctypes.c_void_p(stream)),
            "wekws_hip_stream_frontend_push")
        frames = got[:B].tolist()
        if capacity is None:
            feats = feats[:, :max(frames + [0])]
        return feats, frames

    def reset(self, streams=None) -> None:
        ids = list(range(self.num_streams)) if streams is None else [int(s) for s in streams]
        _capi.check(self._lib.wekws_hip_stream_frontend_reset(self._ptr, (ctypes.c_int32 * max(len(ids), 1))(*ids), len(ids)),
                    "wekws_hip_stream_frontend_reset")

    def counts(self, stream: int) -> Tuple[int, int, int, int]:
        """(leftover samples, remembered frames or -1, skip phase, rows delivered) of a stream: host values, no device read."""
        out = (ctypes.c_int32 * 4)()
        _capi.check(self._lib.wekws_hip_stream_frontend_counts(self._ptr, int(stream), out), "wekws_hip_stream_frontend_counts")
        return tuple(int(v) for v in out)


def _resample_handle(orig_freq, new_freq, out_dtype, max_streams, max_chunk, device, lowpass_filter_width=6, rolloff=0.99):
    if out_dtype not in (torch.float32, torch.int16):
        raise ValueError("out_dtype must be torch.float32 or torch.int16")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the resampler runs on the MI355X HIP path only (no CPU fallback)")
    cfg = _capi.ResampleCfg()
    cfg.orig_freq, cfg.new_freq = int(orig_freq), int(new_freq)
    cfg.lowpass_filter_width, cfg.rolloff = int(lowpass_filter_width), float(rolloff)
    cfg.out_dtype = 1 if out_dtype == torch.int16 else 0
    cfg.max_streams, cfg.max_chunk = int(max_streams), int(max_chunk)
    cfg.device = device.index if device.index is not None else torch.cuda.current_device()
    lib = _capi.load()
    ptr = ctypes.c_void_p()
    _capi.check(lib.wekws_hip_resample_create(ctypes.byref(cfg), ctypes.byref(ptr)), "wekws_hip_resample_create")
    return lib, ptr, torch.device("cuda", cfg.device)


class Resample:
    """``torchaudio.transforms.Resample(orig_freq, new_freq)`` with its defaults (sinc_interp_hann, lowpass_filter_width 6,
    rolloff 0.99: the `resample` step of wekws/dataset/processor.py:83-103) on the device.

        pcm16k = Resample(44100)(pcm)           # pcm (B, nsamp) float32 or int16 on the device -> (B, ceil(nsamp 16000 / 44100))
        feats = Mfcc()(pcm16k)

    ``lengths``: the valid samples of each row (host integers); a row's output is zero past its own count, and the counts
    are returned with it.  ``out_dtype=torch.int16`` rounds (half to even) and saturates."""

    def __init__(self, orig_freq: int, new_freq: int = 16000, device="cuda", out_dtype=torch.float32):
        self.orig_freq, self.new_freq, self.out_dtype = int(orig_freq), int(new_freq), out_dtype
        self._ptr = ctypes.c_void_p()
        self._lib, self._ptr, self.device = _resample_handle(orig_freq, new_freq, out_dtype, 0, 0, device)

    def __del__(self):
        try:
            if self._ptr:
                self._lib.wekws_hip_resample_destroy(self._ptr)
                self._ptr = ctypes.c_void_p()
        except Exception:
            pass

    def num_samples(self, nsamp: int) -> int:
        return int(self._lib.wekws_hip_resample_num_samples(self.orig_freq, self.new_freq, int(nsamp)))

    def __call__(self, pcm: torch.Tensor, lengths=None):
        if not torch.is_tensor(pcm) or pcm.dim() != 2 or not pcm.is_cuda or pcm.dtype not in (torch.float32, torch.int16):
            raise ValueError("pcm must be a (B, nsamp) float32 or int16 tensor on a ROCm device")
        pcm = pcm.contiguous()
        B, n = int(pcm.size(0)), int(pcm.size(1))
        ns = None
        if lengths is not None:
            ns = np.ascontiguousarray(np.clip(np.asarray([int(v) for v in lengths], dtype=np.int64), -1, 2 ** 31 - 1), dtype=np.int32)
            if ns.shape != (B,):
                raise ValueError("lengths must have one entry per row of pcm")
        m = self.num_samples(n)
        out = torch.empty((B, m), dtype=self.out_dtype, device=pcm.device)
        if B:
            stream = torch.cuda.current_stream(pcm.device).cuda_stream
            fn = self._lib.wekws_hip_resample_compute if pcm.dtype == torch.float32 else self._lib.wekws_hip_resample_compute_i16
            _capi.check(fn(self._ptr, pcm.data_ptr() if n else None, B, n, ns.ctypes.data if ns is not None else None,
                           out.data_ptr() if m else None, m, ctypes.c_void_p(stream)), "wekws_hip_resample_compute")
        if lengths is None:
            return out
        return out, [self.num_samples(int(v)) for v in ns]


class StreamingResampler:
    """``Resample`` for ``num_streams`` streams at once, chunk by chunk (wekws_hip_resample_push): int16 chunks of any subset
    of the streams go in, each row's new samples at ``new_freq`` come out.  A stream's outputs, ended by ``flush=True``, are
    the one-shot result of its whole signal bit for bit; an output is emitted by the first push after which every tap that
    can contribute to it lies on a received sample.

        rs = StreamingResampler(4096, 48000, max_chunk=14400)
        out, counts = rs.push(pcm)              # pcm (B, nmax) int16 on the device: row b continues stream b"""

    def __init__(self, num_streams: int, orig_freq: int, new_freq: int = 16000, max_chunk: int = 48000, out_dtype=torch.int16,
                 device="cuda"):
        self.num_streams, self.max_chunk = int(num_streams), int(max_chunk)
        self.orig_freq, self.new_freq, self.out_dtype = int(orig_freq), int(new_freq), out_dtype
        self._ptr = ctypes.c_void_p()
        self._lib, self._ptr, self.device = _resample_handle(orig_freq, new_freq, out_dtype, num_streams, max_chunk, device)

    __del__ = Resample.__del__
    _ABI = "wekws_hip_resample_"                # the entry points the methods below call: _push, _max_out, _reset, _counts

    def _fn(self, name):
        return getattr(self._lib, self._ABI + name)

    def max_out(self, nmax: int, flush: bool = False) -> int:
        """A row capacity that always suffices for chunks of up to ``nmax`` samples."""
        return int(self._fn("max_out")(self._ptr, int(nmax), int(bool(flush))))

    def push(self, pcm, samples=None, streams=None, flush: bool = False, capacity: Optional[int] = None):
        """``pcm``: a (B, nmax) int16 device tensor, or a list of ``bytes`` / int16 arrays (uploaded as ONE padded tensor);
        ``samples`` / ``streams`` as for StreamingFrontEnd.push.  Returns ``(out, counts)``: out (B, max(counts)) on the
        device (``capacity`` columns if given), zero past each row's count; counts a host list.  ``flush`` also emits the
        rows' tails and ends their streams (until ``reset``)."""
        if not torch.is_tensor(pcm):
            arrs = [np.frombuffer(c, dtype="<i2") if isinstance(c, (bytes, bytearray, memoryview)) else np.asarray(c) for c in pcm]
            if any(a.dtype != np.int16 or a.ndim != 1 for a in arrs):
                raise ValueError("chunks must be bytes or 1-d int16 arrays")
            if samples is None:
                samples = [int(a.size) for a in arrs]
            host = np.zeros((len(arrs), max([int(a.size) for a in arrs] + [0])), dtype=np.int16)
            for i, a in enumerate(arrs):
                host[i, :a.size] = a
            pcm = torch.from_numpy(host).to(self.device)
        if pcm.dim() != 2 or not pcm.is_cuda or pcm.dtype != torch.int16:
            raise ValueError("pcm must be a (B, nmax) int16 tensor on a ROCm device")
        pcm = pcm.contiguous()
        B, nmax = int(pcm.size(0)), int(pcm.size(1))
        ids, ns = self._rows(B, streams, samples, lambda: np.full(B, nmax, dtype=np.int32))
        return self._launch("push", pcm, nmax, nmax, ids, ns, flush, capacity)

    @staticmethod
    def _rows(B, streams, samples, default_samples):
        """``streams`` / ``samples`` of a push as int32 arrays of B entries (out of range stays out of range: EINVAL)."""
        if streams is None:
            ids = np.arange(B, dtype=np.int32)
        elif isinstance(streams, np.ndarray) and streams.dtype.kind in "iu":            # (thousands of rows: no Python loop)
            ids = streams.astype(np.int64)
        else:
            ids = np.asarray([int(s) for s in streams], dtype=np.int64)
        if samples is None:
            ns = default_samples()
        elif isinstance(samples, np.ndarray) and samples.dtype.kind in "iu":            # (thousands of rows: no Python loop)
            ns = samples.astype(np.int64)
        else:
            ns = np.asarray([int(n) for n in samples], dtype=np.int64)
        if ids.shape != (B,) or ns.shape != (B,):
            raise ValueError("streams / samples must have one entry per row of pcm")
        lim = np.iinfo(np.int32)
        return (np.ascontiguousarray(np.clip(ids, lim.min, lim.max), dtype=np.int32),
                np.ascontiguousarray(np.clip(ns, lim.min, lim.max), dtype=np.int32))

    def _launch(self, entry, pcm, width, nmax, ids, ns, flush, capacity):
        """The push ``entry`` on pcm (B, width) -- width in the entry point's unit, nmax the most samples of a row."""
        B = int(pcm.size(0))
        cap = self.max_out(nmax, flush) if capacity is None else int(capacity)
        out = torch.empty((B, cap), dtype=self.out_dtype, device=pcm.device)
        got = np.zeros(max(B, 1), dtype=np.int32)
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        _capi.check(self._fn(entry)(
            self._ptr, pcm.data_ptr() if width else None, B, width, ids.ctypes.data if B else None, ns.ctypes.data if B else None,
            int(bool(flush)), out.data_ptr() if cap else None, cap, got.ctypes.data, ctypes.c_void_p(stream)),
            self._ABI + entry)
        counts = got[:B].tolist()
        if capacity is None:
            out = out[:, :max(counts + [0])]
        return out, counts

    def reset(self, streams=None) -> None:
        ids = list(range(self.num_streams)) if streams is None else [int(s) for s in streams]
        _capi.check(self._fn("reset")(self._ptr, (ctypes.c_int32 * max(len(ids), 1))(*ids), len(ids)),
                    self._ABI + "reset")

    def counts(self, stream: int) -> Tuple[int, int, int, int]:
        """(samples received, samples emitted, samples kept on the device, flushed) of a stream: host values, no device read."""
        out = (ctypes.c_int64 * 4)()
        _capi.check(self._fn("counts")(self._ptr, int(stream), out), self._ABI + "counts")
        return tuple(int(v) for v in out)


def _resample_bank_handle(orig_freqs, new_freq, out_dtype, max_streams, max_chunk, device, lowpass_filter_width=6, rolloff=0.99):
    if out_dtype not in (torch.float32, torch.int16):
        raise ValueError("out_dtype must be torch.float32 or torch.int16")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the resampler runs on the MI355X HIP path only (no CPU fallback)")
    members = [_bank_pair(m) for m in orig_freqs]
    rates = [r for r, _ in members]
    cfg = _capi.ResampleCfg()
    cfg.orig_freq, cfg.new_freq = (rates[0] if rates else 0), int(new_freq)
    cfg.lowpass_filter_width, cfg.rolloff = int(lowpass_filter_width), float(rolloff)
    cfg.out_dtype = 1 if out_dtype == torch.int16 else 0
    cfg.max_streams, cfg.max_chunk = int(max_streams), int(max_chunk)
    cfg.device = device.index if device.index is not None else torch.cuda.current_device()
    lib = _capi.load()
    ptr = ctypes.c_void_p()
    arr = (ctypes.c_int32 * max(len(rates), 1))(*rates)
    if all(e == "s16" for _, e in members):
        _capi.check(lib.wekws_hip_resample_bank_create(ctypes.byref(cfg), arr, len(rates), ctypes.byref(ptr)),
                    "wekws_hip_resample_bank_create")
    else:
        encs = (ctypes.c_int32 * len(members))(*[ENCODINGS.index(e) for _, e in members])
        _capi.check(lib.wekws_hip_resample_bank_create_wire(ctypes.byref(cfg), arr, encs, len(rates), ctypes.byref(ptr)),
                    "wekws_hip_resample_bank_create_wire")
    return lib, ptr, torch.device("cuda", cfg.device), rates, members


# the wire encodings of a bank member (enum wekws_hip_wire, in its order) and the bytes of one sample
ENCODINGS = ("s16", "mulaw", "alaw", "u8", "f32")
_WIRE_BYTES = {"s16": 2, "mulaw": 1, "alaw": 1, "u8": 1, "f32": 4}
_WIRE_DTYPE = {"s16": np.dtype("<i2"), "mulaw": np.dtype(np.uint8), "alaw": np.dtype(np.uint8), "u8": np.dtype(np.uint8),
               "f32": np.dtype("<f4")}


def _bank_pair(member):
    """A bank member as ``(rate, encoding)``: an int rate means ``(rate, "s16")``."""
    if isinstance(member, (tuple, list)):
        if len(member) != 2 or member[1] not in ENCODINGS:
            raise ValueError(f"a bank member is a rate or a (rate, encoding) pair with an encoding of {ENCODINGS}, not {member!r}")
        return int(member[0]), str(member[1])
    return int(member), "s16"


def _bank_member(members, key) -> int:
    """The index of ``key`` (a rate, meaning (rate, "s16"), or a (rate, encoding) pair) among the bank's (rate, encoding) pairs."""
    try:
        return members.index(_bank_pair(key))
    except ValueError:
        shown = tuple(r if e == "s16" else (r, e) for r, e in members)
        what = f"rate {key}" if not isinstance(key, (tuple, list)) else f"{tuple(key)}"
        raise ValueError(f"{what} is not in the bank {shown}") from None


class ResampleBank:
    """``Resample`` for a batch whose rows have DIFFERENT source rates (the reference resamples per utterance,
    wekws/dataset/processor.py:94-103), in one launch: a bank of up to 16 source rates and one target rate.

        bank = ResampleBank([8000, 16000, 44100, 48000])
        out, counts = bank(pcm, rate_of_row)     # pcm (B, nsamp) float32 or int16 on the device; rate_of_row: Hz, one per row

    Row b equals ``Resample(rate_of_row[b])`` of that row bit for bit: ``counts[b]`` samples, zeros behind them.  ``lengths``:
    the valid samples of each row (default: all).  A rate that is not in the bank raises ``ValueError``.

    A member may also be a ``(rate, encoding)`` pair, the encoding one of ``ENCODINGS``: the bytes the audio arrives in (G.711
    mu-law / A-law, unsigned 8-bit, float32 at unit scale), decoded to int16 inside the resampler's fetch.

        bank = ResampleBank([(8000, "mulaw"), 16000, (48000, "f32")])
        out, counts = bank(wire, [(8000, "mulaw"), 16000, (48000, "f32")])     # wire (B, row_bytes) uint8 on the device

    Row b of a uint8 tensor holds ``lengths[b]`` samples of its member's encoding from its first byte (default: as many as the row
    holds; ``row_bytes`` a multiple of 4) and equals the int16 call on the decoded samples bit for bit."""

    def __init__(self, orig_freqs, new_freq: int = 16000, device="cuda", out_dtype=torch.float32):
        self.new_freq, self.out_dtype = int(new_freq), out_dtype
        self._ptr = ctypes.c_void_p()
        self._lib, self._ptr, self.device, self.orig_freqs, self.members = _resample_bank_handle(orig_freqs, new_freq, out_dtype,
                                                                                                 0, 0, device)

    def __del__(self):
        try:
            if self._ptr:
                self._lib.wekws_hip_resample_bank_destroy(self._ptr)
                self._ptr = ctypes.c_void_p()
        except Exception:
            pass

    def num_samples(self, rate, nsamp: int) -> int:
        return int(self._lib.wekws_hip_resample_num_samples(_bank_pair(rate)[0], self.new_freq, int(nsamp)))

    def __call__(self, pcm: torch.Tensor, rate_of_row, lengths=None):
        if not torch.is_tensor(pcm) or pcm.dim() != 2 or not pcm.is_cuda or pcm.dtype not in (torch.float32, torch.int16, torch.uint8):
            raise ValueError("pcm must be a (B, nsamp) float32 or int16 tensor, or (B, row_bytes) uint8 wire bytes, on a ROCm device")
        pcm = pcm.contiguous()
        wire = pcm.dtype == torch.uint8
        B, n = int(pcm.size(0)), int(pcm.size(1))               # (n: samples of a row, or bytes of a wire row)
        members = np.ascontiguousarray([_bank_member(self.members, r) for r in rate_of_row], dtype=np.int32)
        if members.shape != (B,):
            raise ValueError("rate_of_row must have one entry per row of pcm")
        holds = [n // _WIRE_BYTES[self.members[m][1]] if wire else n for m in members]      # samples a row has room for
        if lengths is None:
            ns = np.asarray(holds, dtype=np.int32).reshape(B)
        else:
            ns = np.ascontiguousarray(np.clip(np.asarray([int(v) for v in lengths], dtype=np.int64), -1, 2 ** 31 - 1), dtype=np.int32)
            if ns.shape != (B,):
                raise ValueError("lengths must have one entry per row of pcm")
        counts = [self.num_samples(self.orig_freqs[m], max(int(v), 0)) for m, v in zip(members, ns)]
        m = max([self.num_samples(r, h) for r, h in set((self.orig_freqs[k], h) for k, h in zip(members, holds))] + [0])
        out = torch.empty((B, m), dtype=self.out_dtype, device=pcm.device)
        if B:
            stream = torch.cuda.current_stream(pcm.device).cuda_stream
            name = "wekws_hip_resample_bank_compute" + {torch.float32: "", torch.int16: "_i16", torch.uint8: "_wire"}[pcm.dtype]
            _capi.check(getattr(self._lib, name)(self._ptr, pcm.data_ptr() if n else None, B, n, ns.ctypes.data, members.ctypes.data,
                                                 out.data_ptr() if m else None, m, ctypes.c_void_p(stream)), name)
        return out, counts


class StreamingResamplerBank(StreamingResampler):
    """``StreamingResampler`` for streams of DIFFERENT source rates: every stream is assigned one rate of the bank
    (``set_rate``; streams start at ``orig_freqs[0]``) and a push is one launch whatever the rates of its rows.

        rs = StreamingResamplerBank(4096, [48000, 16000, 8000], max_chunk=14400)
        rs.set_rate(range(1024, 2048), 8000)
        out, counts = rs.push(pcm, streams=ids)  # row b continues stream ids[b] at that stream's rate

    ``max_chunk`` counts input samples at whatever rate; ``max_out`` is the largest member's.

    Members may be ``(rate, encoding)`` pairs (``ENCODINGS``), e.g. ``[(8000, "mulaw"), 16000, (48000, "f32")]``: the streams of
    such a member arrive as G.711 bytes, unsigned 8-bit or float32 and are decoded inside the same launch.  ``push`` then takes
    a (B, row_bytes) uint8 device tensor -- row b holds ``samples[b]`` samples of its stream's encoding from its first byte,
    ``row_bytes`` a multiple of 4 -- or a list of ``bytes`` / arrays, each read in its stream's encoding (``len // bytes``
    samples) and uploaded as one padded uint8 tensor.  int16 tensors go where they always went and may only carry rows of
    ``"s16"`` streams."""

    _ABI = "wekws_hip_resample_bank_"

    def __init__(self, num_streams: int, orig_freqs, new_freq: int = 16000, max_chunk: int = 48000, out_dtype=torch.int16,
                 device="cuda"):
        self.num_streams, self.max_chunk = int(num_streams), int(max_chunk)
        self.new_freq, self.out_dtype = int(new_freq), out_dtype
        self._ptr = ctypes.c_void_p()
        self._lib, self._ptr, self.device, self.orig_freqs, self.members = _resample_bank_handle(
            orig_freqs, new_freq, out_dtype, num_streams, max_chunk, device)
        self._wire = any(e != "s16" for _, e in self.members)
        self._bytes = np.asarray([_WIRE_BYTES[e] for _, e in self.members], dtype=np.int64)
        self._member_of = np.zeros(self.num_streams, dtype=np.int64)      # the library's own record, mirrored: streams start on member 0

    __del__ = ResampleBank.__del__

    def set_rate(self, streams, rate) -> None:
        """The streams arrive at ``rate`` (Hz, or a ``(rate, encoding)`` pair: a member of the bank) from now on and start over:
        nothing received, nothing kept, not flushed.  A member outside the bank raises ``ValueError``; a bad stream is refused
        and changes no stream."""
        member = _bank_member(self.members, rate)
        ids = list(range(self.num_streams)) if streams is None else [int(s) for s in streams]
        _capi.check(self._lib.wekws_hip_resample_bank_set_rate(self._ptr, (ctypes.c_int32 * max(len(ids), 1))(*ids), len(ids), member),
                    "wekws_hip_resample_bank_set_rate")
        self._member_of[ids] = member

    def encoding_of(self, stream: int) -> str:
        """The encoding (one of ``ENCODINGS``) in which the stream arrives."""
        enc = int(self._lib.wekws_hip_resample_bank_encoding_of(self._ptr, int(stream)))
        if enc < 0:
            _capi.check(enc, "wekws_hip_resample_bank_encoding_of")
        return ENCODINGS[enc]

    def _row_bytes(self, ids):
        """Bytes of one sample of every row's stream (1 for an id outside the streams: the library refuses the row)."""
        ok = (ids >= 0) & (ids < self.num_streams)
        return np.where(ok, self._bytes[self._member_of[np.where(ok, ids, 0)]], 1)

    def push(self, pcm, samples=None, streams=None, flush: bool = False, capacity: Optional[int] = None):
        """As StreamingResampler.push; with members that are not ``"s16"`` also wire bytes (the class's text)."""
        if not self._wire:
            return super().push(pcm, samples, streams, flush, capacity)
        if not torch.is_tensor(pcm):
            chunks = list(pcm)
            ids = np.arange(len(chunks)) if streams is None else np.asarray([int(s) for s in streams], dtype=np.int64)
            if ids.shape != (len(chunks),):
                raise ValueError("streams / samples must have one entry per row of pcm")
            ok = (ids >= 0) & (ids < self.num_streams)
            rows = []
            for c, i, good in zip(chunks, ids, ok):
                enc = self.members[self._member_of[i]][1] if good else "s16"
                if isinstance(c, (bytes, bytearray, memoryview)):
                    a = np.frombuffer(c, dtype=np.uint8)
                    a = a[:a.size // _WIRE_BYTES[enc] * _WIRE_BYTES[enc]]
                else:
                    a = np.asarray(c)
                    if a.ndim != 1 or a.dtype != _WIRE_DTYPE[enc]:
                        raise ValueError(f"a chunk of a {enc!r} stream must be bytes or a 1-d {_WIRE_DTYPE[enc].name} array")
                    a = np.ascontiguousarray(a).view(np.uint8)
                rows.append(a)
            if samples is None:
                samples = [int(a.size) // int(b) for a, b in zip(rows, self._row_bytes(ids))]
            host = np.zeros((len(rows), (max([int(a.size) for a in rows] + [0]) + 3) // 4 * 4), dtype=np.uint8)
            for i, a in enumerate(rows):
                host[i, :a.size] = a
            pcm = torch.from_numpy(host).to(self.device)
        if pcm.dtype != torch.uint8:
            return super().push(pcm, samples, streams, flush, capacity)
        if pcm.dim() != 2 or not pcm.is_cuda:
            raise ValueError("pcm must be a (B, row_bytes) uint8 tensor on a ROCm device")
        pcm = pcm.contiguous()
        B, row_bytes = int(pcm.size(0)), int(pcm.size(1))
        ids, ns = self._rows(B, streams, samples, lambda: np.zeros(B, dtype=np.int32))
        if samples is None:                                                          # every row as full as its encoding fills it
            ns = np.ascontiguousarray(row_bytes // self._row_bytes(ids.astype(np.int64)), dtype=np.int32)
        nmax = int(np.clip(ns, 0, row_bytes).max()) if B else 0
        return self._launch("push_wire", pcm, row_bytes, nmax, ids, ns, flush, capacity)

    def rate_of(self, stream: int) -> int:
        """The rate in Hz at which the stream arrives."""
        rate = int(self._lib.wekws_hip_resample_bank_rate_of(self._ptr, int(stream)))
        if rate <= 0:
            _capi.check(rate, "wekws_hip_resample_bank_rate_of")
        return rate
