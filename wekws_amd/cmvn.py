"""Global CMVN statistics on the device: the accumulation of the reference's ``tools/compute_cmvn_stats.py`` (:26-72, :128-151)
for features that ``frontend.Fbank`` / ``frontend.Mfcc`` left on the device.  A thin host wrapper over the C ABI
(wekws_hip_cmvn_stats_*); no CPU fallback.

    st = CmvnStats(80)
    for pcm, frames in batches:                    # zero-padded batches, frames per row from Fbank.num_frames
        st.update(fbank(pcm), frames)
    st.save("data/train/global_cmvn")              # {"mean_stat", "var_stat", "frame_num"}: what utils.cmvn.load_cmvn reads

The sums are accumulated in double (the reference: float32), so they are within ``N 2^-53 sum|term|`` of the exact sums over the
``N`` frames since the last reset; a sum the reference's float32 would overflow stays finite.  Shards of a data set (the ranks of
``parallel.shard_range``) each keep a ``CmvnStats``; ``merge_cmvn_stats`` adds their results on the host."""
from __future__ import annotations

import ctypes
import json

import numpy as np
import torch

from wekws_amd import _capi

MAX_DIM = 4096


class CmvnStats:
    """Running per-bin sums, sums of squares and the frame count of (B, T, dim) float32 feature batches on a ROCm device.

    ``update(feats, lengths)``: ``lengths`` are the valid frames of each row -- host integers (checked here: one outside
    0..T raises ``ValueError`` and nothing is launched) or an integer tensor on the device (checked by the kernel: such a row
    adds nothing and ``result()`` raises).  ``update`` and ``reset`` are asynchronous on the current stream; ``result()``
    synchronises."""

    def __init__(self, dim: int, device=None):
        self._ptr = ctypes.c_void_p()
        self._lib = _capi.load()
        self.dim = int(dim)
        if not 1 <= self.dim <= MAX_DIM:
            raise ValueError(f"dim must be in 1..{MAX_DIM}")
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise RuntimeError("wekws_amd.cmvn.CmvnStats runs on the MI355X HIP path only (no CPU fallback)")
        idx = device.index if device.index is not None else torch.cuda.current_device()
        _capi.check(self._lib.wekws_hip_cmvn_stats_create(self.dim, idx, ctypes.byref(self._ptr)), "wekws_hip_cmvn_stats_create")
        self.device = torch.device("cuda", idx)

    def __del__(self):
        try:
            if self._ptr:
                self._lib.wekws_hip_cmvn_stats_destroy(self._ptr)
                self._ptr = ctypes.c_void_p()
        except Exception:
            pass

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def update(self, feats: torch.Tensor, lengths=None) -> "CmvnStats":
        if not torch.is_tensor(feats) or feats.dim() != 3 or not feats.is_cuda or feats.dtype != torch.float32:
            raise ValueError("feats must be a (B, T, dim) float32 tensor on a ROCm device")
        if feats.device != self.device:
            raise ValueError(f"feats is on {feats.device}, the statistics on {self.device}")
        B, T, D = (int(v) for v in feats.shape)
        if D != self.dim:
            raise ValueError(f"feats has {D} bins, the statistics {self.dim}")
        feats = feats.contiguous()
        lens = None
        if torch.is_tensor(lengths) and lengths.is_cuda:
            if lengths.shape != (B,) or lengths.is_floating_point() or lengths.device != self.device:
                raise ValueError("lengths must be (B) integers on feats' device")
            lens = lengths if lengths.dtype == torch.int32 else lengths.clamp(-1, 2 ** 31 - 1).to(torch.int32)      # (out of range stays so)
            lens = lens.contiguous()
        elif lengths is not None:
            host = np.asarray(lengths.cpu().numpy() if torch.is_tensor(lengths) else [int(v) for v in lengths], dtype=np.int64)
            if host.shape != (B,):
                raise ValueError("lengths must have one entry per row of feats")
            bad = [int(b) for b in np.nonzero((host < 0) | (host > T))[0]]
            if bad:
                raise ValueError(f"lengths[{bad[0]}] = {int(host[bad[0]])} is outside 0..{T}")
            lens = torch.from_numpy(host.astype(np.int32)).to(self.device)
        if B and T:
            _capi.check(self._lib.wekws_hip_cmvn_stats_update(self._ptr, feats.data_ptr(), B, T, lens.data_ptr() if lens is not None else None,
                                                              self._stream()), "wekws_hip_cmvn_stats_update")
        return self

    def reset(self) -> None:
        _capi.check(self._lib.wekws_hip_cmvn_stats_reset(self._ptr, self._stream()), "wekws_hip_cmvn_stats_reset")

    def read(self):
        """(mean_stat, var_stat) float64 arrays, frame_num, bad_rows -- as they stand, bad rows or not."""
        mean, var = np.empty(self.dim, dtype=np.float64), np.empty(self.dim, dtype=np.float64)
        counts = (ctypes.c_int64 * 2)()
        _capi.check(self._lib.wekws_hip_cmvn_stats_read(self._ptr, mean.ctypes.data, var.ctypes.data, counts, self._stream()),
                    "wekws_hip_cmvn_stats_read")
        return mean, var, int(counts[0]), int(counts[1])

    def result(self) -> dict:
        mean, var, n, bad = self.read()
        if bad:
            raise ValueError(f"{bad} rows had a length outside 0..T and were left out: the statistics are incomplete")
        return {"mean_stat": mean.tolist(), "var_stat": var.tolist(), "frame_num": n}

    def save(self, path: str) -> None:
        save_cmvn_stats(self.result(), path)

    def mean_istd(self) -> np.ndarray:
        return mean_istd(self.result())


def save_cmvn_stats(stats: dict, path: str) -> None:
    """The reference's file (compute_cmvn_stats.py:144-151): Python floats print with every digit, so the file holds the doubles."""
    with open(path, "w") as f:
        f.write(json.dumps({"mean_stat": list(stats["mean_stat"]), "var_stat": list(stats["var_stat"]), "frame_num": int(stats["frame_num"])}))


def mean_istd(stats: dict) -> np.ndarray:
    """(2, dim) float64 [mean, 1 / std] of a ``result()``: ``utils.cmvn.load_cmvn`` of the saved file, bit for bit."""
    n = float(stats["frame_num"])
    mean = np.asarray(stats["mean_stat"], dtype=np.float64) / n
    var = np.asarray(stats["var_stat"], dtype=np.float64) / n - mean * mean
    return np.stack([mean, 1.0 / np.sqrt(np.maximum(var, 1.0e-20))])


def merge_cmvn_stats(results) -> dict:
    """Adds several ``result()`` dicts in list order, in double: shards or ranks of one data set, no collective needed."""
    results = list(results)
    if not results:
        raise ValueError("nothing to merge")
    dim = len(results[0]["mean_stat"])
    mean, var, n = [0.0] * dim, [0.0] * dim, 0
    for r in results:
        if len(r["mean_stat"]) != dim or len(r["var_stat"]) != dim:
            raise ValueError("the results have different numbers of bins")
        mean = [a + float(b) for a, b in zip(mean, r["mean_stat"])]
        var = [a + float(b) for a, b in zip(var, r["var_stat"])]
        n += int(r["frame_num"])
    return {"mean_stat": mean, "var_stat": var, "frame_num": n}
