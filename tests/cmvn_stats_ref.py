"""The yardstick of the global CMVN statistics (wekws_amd/cmvn.py, csrc/cmvn_stats.hip.h): the exact oracle, the bar derived
from it, a restatement of the reference's float32 accumulation, and the cases.

The bar.  For ANY order of summing N terms in double, |computed - exact| <= gamma_(N-1) sum|term| with gamma_n = n u / (1 - n u),
u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), which for N < 9e7 is below N 2^-53 sum|term|.  float64(x) is
exact for a float32 x and so is its square (48 significant bits), so the terms themselves carry no error, and math.fsum of them
is the correctly rounded exact sum.  N is the number of valid frames since the last reset; `units` below is |got - exact| over
N 2^-53 sum|term| per bin, and the bar is 1.  It is not measured from any implementation."""
import math

import numpy as np

U = 2.0 ** -53
KINDS = ("none", "full", "mixed", "zero")


def lengths_of(kind, B, T, seed=0):
    """frames per row: None, all T, mixed (a 0 and a T among them where B allows), all 0"""
    if kind == "none":
        return None
    if kind == "full":
        return [T] * B
    if kind == "zero":
        return [0] * B
    rng = np.random.default_rng(1000 + seed)
    out = [int(v) for v in rng.integers(0, T + 1, size=B)]
    out[0] = T - T // 3                       # (B = 1: a proper part of the row)
    if B > 1:
        out[1] = 0
    if B > 2:
        out[2] = T
    return out


def feats_of(B, T, D, seed=0):
    """features around 10 +- 4, as log-mel energies of int16-scale audio are"""
    rng = np.random.default_rng(seed)
    return (10.0 + 4.0 * rng.standard_normal((B, T, D))).astype(np.float32)


def valid_rows(x, lengths):
    """(N, D) float64: the valid frames of a batch, row by row"""
    B, T, D = x.shape
    lens = [T] * B if lengths is None else [int(v) for v in lengths]
    rows = [x[b, :lens[b]] for b in range(B)]
    return np.concatenate(rows, axis=0).astype(np.float64) if rows else np.zeros((0, D))


def _exact(col):
    """the exact sum of a column of doubles, with IEEE's classes for the non-finite ones"""
    if np.isnan(col).any():
        return math.nan
    pos, neg = bool(np.isposinf(col).any()), bool(np.isneginf(col).any())
    if pos and neg:
        return math.nan
    if pos or neg:
        return math.inf if pos else -math.inf
    return math.fsum(col.tolist())


def oracle(frames):
    """frames (N, D) float64 -> dict of per-bin exact sums and sums of squares, their sum|term| and N"""
    N, D = frames.shape
    with np.errstate(over="ignore", invalid="ignore"):
        sq = frames * frames
    fin = np.where(np.isfinite(frames), frames, 0.0)
    return {"mean_stat": np.asarray([_exact(frames[:, d]) for d in range(D)]), "var_stat": np.asarray([_exact(sq[:, d]) for d in range(D)]),
            "abs_mean": np.asarray([math.fsum(np.abs(fin[:, d]).tolist()) for d in range(D)]),
            "abs_var": np.asarray([math.fsum((fin[:, d] * fin[:, d]).tolist()) for d in range(D)]), "frame_num": int(N)}


def units(got, want, key):
    """per finite bin |got - exact| / (N 2^-53 sum|term|) (0 where both are exact zeros); bins whose oracle is not finite are
    compared by class instead (same_class) and come back as 0 here"""
    got = np.asarray(got, dtype=np.float64)
    exact, scale = want[key], want["abs_" + key.split("_")[0]] * (max(want["frame_num"], 1) * U)
    fin = np.isfinite(exact)
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, exact, 0.0)), 0.0)
    bad = fin & ~np.isfinite(got)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(err == 0.0, 0.0, err / scale)
    return np.where(bad, np.inf, u)


def same_class(got, exact):
    """NaN where the oracle is NaN, the same infinity where it is infinite, finite elsewhere"""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    return bool((np.isnan(got) == np.isnan(exact)).all() and (np.isposinf(got) == np.isposinf(exact)).all() and
                (np.isneginf(got) == np.isneginf(exact)).all())


def inside(result, want):
    """a result dict against the oracle: (worst units of mean_stat, worst units of var_stat, frame_num exact, classes right)"""
    return (float(units(result["mean_stat"], want, "mean_stat").max(initial=0.0)), float(units(result["var_stat"], want, "var_stat").max(initial=0.0)),
            int(result["frame_num"]) == want["frame_num"],
            same_class(result["mean_stat"], want["mean_stat"]) and same_class(result["var_stat"], want["var_stat"]))


def float64_accumulation(x, lengths):
    """a plain numpy accumulation in double, utterance by utterance"""
    B, T, D = x.shape
    lens = [T] * B if lengths is None else lengths
    mean, var, n = np.zeros(D), np.zeros(D), 0
    for b in range(B):
        m = x[b, :lens[b]].astype(np.float64)
        mean += m.sum(axis=0)
        var += (m * m).sum(axis=0)
        n += int(lens[b])
    return {"mean_stat": mean.tolist(), "var_stat": var.tolist(), "frame_num": n}


def reference_float32(x, lengths, batch=20):
    """tools/compute_cmvn_stats.py:26-72 and :128-138: per utterance torch.sum(mat, axis=0) and torch.sum(torch.square(mat), axis=0)
    added in float32 to the batch's accumulators (20 utterances a batch), those added in float32 to the totals"""
    import torch
    B, T, D = x.shape
    lens = [T] * B if lengths is None else lengths
    all_mean, all_var, all_n = torch.zeros(D), torch.zeros(D), 0
    for at in range(0, B, batch):
        mean, var, n = torch.zeros(D), torch.zeros(D), 0
        for b in range(at, min(B, at + batch)):
            mat = torch.from_numpy(np.ascontiguousarray(x[b, :lens[b]]))
            mean += torch.sum(mat, axis=0)
            var += torch.sum(torch.square(mat), axis=0)
            n += mat.shape[0]
        all_mean += mean
        all_var += var
        all_n += n
    return {"mean_stat": list(all_mean.tolist()), "var_stat": list(all_var.tolist()), "frame_num": all_n}


# ---- the host cases: (name, B, T, D, kind of lengths)
CPU_CASES = (("3x7x5", 3, 7, 5, "none"), ("4x300x80", 4, 300, 80, "mixed"), ("2x4096x40", 2, 4096, 40, "full"))

# ---- the device cases, from the plan's tile (frames a workgroup takes: a function of D)
GPU_DIMS = (1, 40, 80, 83, 400, 1030)
GPU_BATCHES = (1, 3, 5)


def tile_frames(D):
    import ctypes
    from wekws_amd import _capi
    out = (ctypes.c_int64 * 3)()
    assert _capi.load().wekws_hip_cmvn_stats_plan(1, 1, int(D), out) == 0, _capi.last_error()
    return int(out[0])


def gpu_cases():
    """(name, B, T, D, kind).  Every D with T in {1, tile - 1, tile, tile + 1, 2 tile + 1}, B and the kind of lengths rotating
    through the list; then every B x kind at the odd width, one frame past a tile."""
    cases, i = [], 0
    for D in GPU_DIMS:
        tile = tile_frames(D)
        for T in sorted({1, tile - 1, tile, tile + 1, 2 * tile + 1} - {0}):
            B, kind = GPU_BATCHES[i % 3], KINDS[(i // 3) % 4]
            cases.append((f"{B}x{T}x{D}-{kind}", B, T, D, kind))
            i += 1
    tile = tile_frames(83)
    for B in GPU_BATCHES:
        for kind in KINDS:
            name = f"{B}x{tile + 1}x83-{kind}"
            if all(c[0] != name for c in cases):
                cases.append((name, B, tile + 1, 83, kind))
    return cases


def is_negative_control(B, T, kind):
    """where a float32 sum over every frame of the tensor can be held against the same bar: all frames valid, and enough of them
    that the exact sums need more than float32's 24 bits (one frame's sum is exact in any format)"""
    return kind in ("none", "full") and B * T >= 16
