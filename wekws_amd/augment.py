"""The augmentation stages of the data pipeline on the device, between ``frontend.Resample`` and ``frontend.Fbank``:
``add_reverb`` (wekws/dataset/processor.py:374-392), ``add_noise`` (395-430) and ``spec_aug`` (206-240).  Thin host wrappers
over the C ABI (wekws_hip_reverb_*, wekws_hip_noise_*, wekws_hip_spec_mask); no CPU fallback.

What the reference draws at random is drawn on the host and passed in: ``draw_reverb``, ``draw_noise`` and ``draw_spec_aug``
consume a ``random.Random`` in exactly the reference's call order, so a seeded reference run and a seeded run of these make the
same choices.

    rv, nz = Reverb(rirs), AddNoise(noises, pcm_scale=1.0)
    wet = rv(pcm, draw_reverb(rng, rv.num_rirs, 0.5, B), lengths)
    noisy = nz(wet, *draw_noise(rng, keys, nz.lengths, lengths, 0.5), lengths=lengths)
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from wekws_amd import _capi

SNR_RANGES = (("noise", (0, 15)), ("speech", (5, 30)), ("music", (5, 15)))      # by the key's prefix; anything else: 0..15


def _bank(arrays, lengths, what):
    """(R, max_len) float32 and (R) int32 of a list of 1-d arrays, or of a padded 2-d array with ``lengths``"""
    if isinstance(arrays, np.ndarray) and arrays.ndim == 2 or torch.is_tensor(arrays):
        bank = np.ascontiguousarray(arrays.detach().cpu().numpy() if torch.is_tensor(arrays) else arrays, dtype=np.float32)
        if bank.ndim != 2:
            raise ValueError(f"{what} must be (R, max_len) or a list of 1-d arrays")
        lens = np.full(bank.shape[0], bank.shape[1], dtype=np.int64) if lengths is None else np.asarray([int(v) for v in lengths], dtype=np.int64)
    else:
        rows = [np.asarray(a, dtype=np.float32).reshape(-1) for a in arrays]
        if lengths is not None:
            raise ValueError(f"lengths go with a padded (R, max_len) array; a list of {what} carries its own")
        lens = np.asarray([r.size for r in rows], dtype=np.int64)
        bank = np.zeros((len(rows), max([int(n) for n in lens] + [1])), dtype=np.float32)
        for i, r in enumerate(rows):
            bank[i, :r.size] = r
    if lens.shape != (bank.shape[0],):
        raise ValueError("lengths must have one entry per row")
    return bank, np.ascontiguousarray(np.clip(lens, -1, 2 ** 31 - 1), dtype=np.int32)


def _device_index(device) -> int:
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the augmentation stages run on the MI355X HIP path only (no CPU fallback)")
    return device.index if device.index is not None else torch.cuda.current_device()


def _rows(values, B, what, dtype=np.int32):
    a = np.asarray(values if isinstance(values, np.ndarray) else list(values), dtype=np.float64 if dtype == np.float64 else np.int64)
    if a.shape != (B,):
        raise ValueError(f"{what} must have one entry per row of pcm")
    if dtype == np.int32:
        a = np.clip(a, np.iinfo(np.int32).min, np.iinfo(np.int32).max)      # (out of range stays out of range: EINVAL)
    return np.ascontiguousarray(a, dtype=dtype)


def _masks(m, B):
    a = np.asarray(m, dtype=np.int64)
    if B == 0:
        return np.zeros((0, 0, 2), dtype=np.int32)
    if a.size % (2 * B):
        raise ValueError("masks must be (B, count, 2) [start, end) pairs")
    return np.ascontiguousarray(a.reshape(B, a.size // (2 * B), 2).clip(-1, 2 ** 31 - 1), dtype=np.int32)


def _check_pcm(pcm):
    if not torch.is_tensor(pcm) or pcm.dim() != 2 or not pcm.is_cuda or pcm.dtype != torch.float32:
        raise ValueError("pcm must be a (B, nsamp) float32 tensor on a ROCm device")
    return pcm.contiguous()


class _Handle:
    _destroy = ""

    def __del__(self):
        try:
            if self._ptr:
                getattr(self._lib, self._destroy)(self._ptr)
                self._ptr = ctypes.c_void_p()
        except Exception:
            pass


class Reverb(_Handle):
    """``signal.convolve(audio, rir / sqrt(sum(rir**2)), 'full')[:len(audio)]`` for a batch, each row with the RIR of its
    choice out of a bank that stays on the device (as partition spectra: ``spectra_bytes``).

        wet = Reverb(rirs)(pcm, rir_of_row, lengths)       # rir_of_row[b] = -1: row b is copied bit for bit

    ``rirs``: a list of 1-d arrays, or (R, max_len) with ``lengths``.  ``pcm`` (B, nsamp) float32 on the device in any scale.
    Samples at or past a row's length come back as zeros."""
    _destroy = "wekws_hip_reverb_destroy"

    def __init__(self, rirs, lengths=None, device="cuda"):
        self._ptr = ctypes.c_void_p()
        self._lib = _capi.load()
        bank, lens = _bank(rirs, lengths, "rirs")
        idx = _device_index(device)
        _capi.check(self._lib.wekws_hip_reverb_create(bank.ctypes.data, lens.ctypes.data, bank.shape[0], bank.shape[1], idx,
                                                      ctypes.byref(self._ptr)), "wekws_hip_reverb_create")
        self.device = torch.device("cuda", idx)
        self.lengths = [int(n) for n in lens]
        self.num_rirs = len(self.lengths)
        self.hop = int(self._lib.wekws_hip_reverb_hop())
        self.spectra_bytes = sum(-(-n // self.hop) for n in self.lengths) * (self.hop + 1) * 8

    def workspace_bytes(self, B: int, nmax: int) -> int:
        return int(self._lib.wekws_hip_reverb_workspace_bytes(self._ptr, int(B), int(nmax)))

    def __call__(self, pcm: torch.Tensor, rir_of_row, lengths=None, out=None) -> torch.Tensor:
        pcm = _check_pcm(pcm)
        B, n = int(pcm.size(0)), int(pcm.size(1))
        rir = _rows(rir_of_row, B, "rir_of_row")
        ns = None if lengths is None else _rows(lengths, B, "lengths")
        if out is None:
            out = torch.empty_like(pcm) if lengths is None else torch.zeros_like(pcm)
        elif not torch.is_tensor(out) or out.shape != pcm.shape or out.dtype != torch.float32 or out.device != pcm.device or \
                not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor of pcm's shape on pcm's device")
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        _capi.check(self._lib.wekws_hip_reverb_apply(
            self._ptr, pcm.data_ptr() if B * n else None, B, n, ns.ctypes.data if ns is not None else None,
            rir.ctypes.data if B else None, out.data_ptr() if B * n else None, ctypes.c_void_p(stream)), "wekws_hip_reverb_apply")
        return out


class AddNoise(_Handle):
    """``audio + sqrt(10 ** ((audio_db - noise_db - snr) / 10)) * noise`` for a batch, each row with the noise, the start and
    the SNR of its choice; the noises (float32 in int16 scale, as ``wavfile.read`` gives them) stay on the device.

        noisy = AddNoise(noises, pcm_scale=1.0)(pcm, noise_of_row, start, snr_db, lengths)

    ``pcm_scale``: 1 for samples in [-1, 1] (what the reference's ``add_noise`` sees), 32768 for int16-scale floats.  Row b
    takes ``noise[(start[b] + n) % len(noise)]``; ``noise_of_row[b] = -1`` copies it.  ``inplace=True`` writes into ``pcm``."""
    _destroy = "wekws_hip_noise_destroy"

    def __init__(self, noises, lengths=None, pcm_scale: float = 1.0, device="cuda"):
        self._ptr = ctypes.c_void_p()
        self._lib = _capi.load()
        bank, lens = _bank(noises, lengths, "noises")
        idx = _device_index(device)
        _capi.check(self._lib.wekws_hip_noise_create(bank.ctypes.data, lens.ctypes.data, bank.shape[0], bank.shape[1], idx,
                                                     ctypes.byref(self._ptr)), "wekws_hip_noise_create")
        self.device = torch.device("cuda", idx)
        self.lengths = [int(n) for n in lens]
        self.pcm_scale = float(pcm_scale)

    def __call__(self, pcm: torch.Tensor, noise_of_row, start, snr_db, lengths=None, inplace: bool = False) -> torch.Tensor:
        pcm = _check_pcm(pcm)
        B, n = int(pcm.size(0)), int(pcm.size(1))
        which, st = _rows(noise_of_row, B, "noise_of_row"), _rows(start, B, "start")
        snr = _rows(snr_db, B, "snr_db", np.float64)
        ns = None if lengths is None else _rows(lengths, B, "lengths")
        out = pcm if inplace else (pcm.clone() if lengths is not None else torch.empty_like(pcm))
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        _capi.check(self._lib.wekws_hip_noise_mix(
            self._ptr, pcm.data_ptr() if B * n else None, B, n, ns.ctypes.data if ns is not None else None,
            which.ctypes.data if B else None, st.ctypes.data if B else None, snr.ctypes.data if B else None, self.pcm_scale,
            out.data_ptr() if B * n else None, ctypes.c_void_p(stream)), "wekws_hip_noise_mix")
        return out


def spec_aug(feats: torch.Tensor, t_masks, f_masks, lengths=None, inplace: bool = False) -> torch.Tensor:
    """The masks of ``spec_aug``: within row b's frames, frames ``t_masks[b, i, 0] .. t_masks[b, i, 1]`` and bins
    ``f_masks[b, i, 0] .. f_masks[b, i, 1]`` (end exclusive, already clipped) become 0; everything else is copied.
    ``feats`` (B, T, F) float32 on the device; the masks are host integers of shape (B, nt, 2) and (B, nf, 2)."""
    if not torch.is_tensor(feats) or feats.dim() != 3 or not feats.is_cuda or feats.dtype != torch.float32:
        raise ValueError("feats must be a (B, T, F) float32 tensor on a ROCm device")
    feats = feats.contiguous()
    B, T, F = (int(v) for v in feats.shape)
    tm, fm = _masks(t_masks, B), _masks(f_masks, B)
    ns = None if lengths is None else _rows(lengths, B, "lengths")
    out = feats if inplace else torch.empty_like(feats)
    stream = torch.cuda.current_stream(feats.device).cuda_stream
    _capi.check(_capi.load().wekws_hip_spec_mask(
        feats.data_ptr() if feats.numel() else None, B, T, F, ns.ctypes.data if ns is not None else None,
        tm.ctypes.data if tm.size else None, tm.shape[1], fm.ctypes.data if fm.size else None, fm.shape[1],
        out.data_ptr() if feats.numel() else None, ctypes.c_void_p(stream)), "wekws_hip_spec_mask")
    return out


# ---- the reference's draws, in its call order
def draw_reverb(rng, num_rirs: int, aug_prob: float, B: int):
    """rir_of_row for B rows: ``aug_prob > random.random()``, then ``LmdbData.random_one``'s ``randint(0, R - 1)``."""
    out = []
    for _ in range(B):
        out.append(rng.randint(0, num_rirs - 1) if aug_prob > rng.random() else -1)
    return out


def snr_range(key: str):
    for prefix, r in SNR_RANGES:
        if key.startswith(prefix):
            return r
    return (0, 15)


def draw_noise(rng, keys, noise_lengths, audio_lengths, aug_prob: float):
    """(noise_of_row, start, snr_db) for rows of ``audio_lengths`` samples: the ``aug_prob`` draw, ``random_one``, then
    ``randint(0, nlen - len)`` only where the noise is longer than the row, then ``uniform`` over the key's SNR range."""
    which, start, snr = [], [], []
    for alen in audio_lengths:
        if not aug_prob > rng.random():
            which.append(-1); start.append(0); snr.append(0.0)
            continue
        i = rng.randint(0, len(keys) - 1)
        lo, hi = snr_range(keys[i])
        nlen = int(noise_lengths[i])
        which.append(i)
        start.append(rng.randint(0, nlen - int(alen)) if nlen > int(alen) else 0)
        snr.append(rng.uniform(lo, hi))
    return which, start, snr


def draw_spec_aug(rng, lengths, F: int, num_t_mask: int = 2, num_f_mask: int = 2, max_t: int = 50, max_f: int = 10):
    """(t_masks (B, num_t_mask, 2), f_masks (B, num_f_mask, 2)) for rows of ``lengths`` frames and F bins, clipped as the
    reference clips them: per row the time masks first, each ``randint(0, T - 1)`` then ``randint(1, max_t)``."""
    B = len(lengths)
    tm = np.zeros((B, num_t_mask, 2), dtype=np.int32)
    fm = np.zeros((B, num_f_mask, 2), dtype=np.int32)
    for b, T in enumerate(lengths):
        for i in range(num_t_mask):
            s = rng.randint(0, int(T) - 1)
            tm[b, i] = s, min(int(T), s + rng.randint(1, max_t))
        for i in range(num_f_mask):
            s = rng.randint(0, F - 1)
            fm[b, i] = s, min(F, s + rng.randint(1, max_f))
    return tm, fm
