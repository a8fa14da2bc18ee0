#!/usr/bin/env python3
"""Generate tests/golden/stream_frontend_golden.npz by driving the reference's own ``KeyWordSpotter.accept_wave``
(wekws/bin/stream_kws_ctc.py:335-398) with ``kaldi.fbank`` replaced by a framing-only stand-in.  Build container only:

    WEKWS_REFERENCE=<reference checkout> python tests/golden/make_stream_frontend_golden.py

The stand-in returns, per snip-edges frame, the raw samples at four fixed offsets of the frame; the PCM is a ramp
(sample g has the value g), so every recorded value names its global sample and with it the global frame.  Per push the
file holds the returned matrix (or the None / assertion marker) and the three counts the spotter carries: leftover
samples, remembered feature frames, skip phase.  Integers only.

Arrays, per case <c>:  cfg/<c> = [L, S, left, right, skip];  n/<c> pushes;  kind/<c> rows of each push (-1 = None,
-2 = the reference's assertion: the schedule ends there);  counts/<c> (pushes, 3) after each push (fr: -1 = None);
rows/<c> (sum of rows, (left + right + 1) * 4) the matrices, concatenated.  offsets = the four offsets per frame length.
"""
from __future__ import annotations

import os
import struct
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
RATE = 16000


def offsets(L):
    return [0, 1, L // 2, L - 1]


def load_reference():
    ref = os.environ.get("WEKWS_REFERENCE")
    if not ref:
        sys.exit("set WEKWS_REFERENCE to the reference checkout")
    if ref not in sys.path:
        sys.path.insert(0, ref)
    for name in ("librosa", "torchaudio", "torchaudio.compliance", "torchaudio.compliance.kaldi"):
        sys.modules.setdefault(name, types.ModuleType(name))
    ml = types.ModuleType("tools.make_list")
    for name in ("query_token_set", "read_lexicon", "read_token"):
        setattr(ml, name, lambda *a, **k: None)
    sys.modules.setdefault("tools", types.ModuleType("tools"))
    sys.modules["tools.make_list"] = ml
    import wekws.bin.stream_kws_ctc as skc

    def framing_only(wave, num_mel_bins, frame_length, frame_shift, dither, energy_floor, sample_frequency):
        """kaldi.fbank's framing (snip_edges) without its arithmetic: frame k -> the samples at offsets(L) of it."""
        L, S = int(frame_length * sample_frequency / 1000), int(frame_shift * sample_frequency / 1000)
        x = wave[0]
        nf = 0 if x.numel() < L else 1 + (x.numel() - L) // S
        out = torch.zeros(nf, 4, dtype=torch.float32)
        for k in range(nf):
            for j, o in enumerate(offsets(L)):
                out[k, j] = x[k * S + o]
        return out

    skc.kaldi.fbank = framing_only
    return skc


def make_spotter(skc, L_ms, S_ms, left, right, skip):
    kws = object.__new__(skc.KeyWordSpotter)
    torch.nn.Module.__init__(kws)
    kws.sample_rate = RATE
    kws.wave_remained = np.array([])
    kws.num_mel_bins = 4
    kws.frame_length, kws.frame_shift = L_ms, S_ms
    kws.downsampling = skip
    kws.context_expansion = left > 0 or right > 0
    kws.left_context, kws.right_context = left, right
    kws.feature_remained = None
    kws.feats_ctx_offset = 0
    kws.device = torch.device("cpu")
    return kws


def random_sizes(rng, total, hi=5000):
    out, left = [], total
    special = [0, 1, 2, 159, 160, 161, 399, 400, 401]
    while left > 0:
        n = int(rng.choice(special)) if rng.random() < 0.4 else int(rng.integers(1, hi))
        n = min(n, left)
        out.append(n)
        left -= n
    return out


def avoid_assert(L, S, right, pushes):
    """Lengthen a push that would give the reference no more frames than its right context (only r = 1 can: 400 <= tot <
    560 at 400 / 160) by whole frame shifts, so that a schedule runs to its end.  Framing arithmetic only."""
    out, rem = [], 0
    for n in pushes:
        while True:
            tot = rem + n
            nf = 0 if tot < L else 1 + (tot - L) // S
            if right == 0 or tot < L * right or nf > right:
                break
            n += S
        out.append(n)
        rem = tot if tot < L * right else tot - nf * S
    return out


def cases(rng):
    """(name, L_ms, S_ms, left, right, skip, pushes)."""
    cs = []
    mixed = [0, 1, 399, 1, 159, 160, 161, 4800, 0, 777, 1, 2, 3001, 4800, 401, 1601, 0, 4800, 333]
    for left, right, skip in ((0, 0, 1), (0, 0, 3), (2, 2, 3), (1, 1, 2), (2, 2, 1), (3, 3, 2)):
        tag = f"l{left}r{right}s{skip}"
        # (1, 1, x): a push that leaves 400 <= tot < 560 trips the assertion; avoid_assert lengthens it
        cs.append((f"mixed_{tag}", 25, 10, left, right, skip, avoid_assert(400, 160, right, mixed)))
        cs.append((f"steady_{tag}", 25, 10, left, right, skip, [4800] * 6))
        cs.append((f"random_{tag}", 25, 10, left, right, skip, avoid_assert(400, 160, right, random_sizes(rng, 28000))))
    # pushes that are held (right >= 1: tot < L * right), odd sizes
    cs.append(("held_l2r2s3", 25, 10, 2, 2, 3, [100, 101, 1, 0, 333, 264, 1, 4800, 37, 500, 300, 4800]))
    cs.append(("held_l3r3s2", 25, 10, 3, 3, 2, [399, 400, 400, 1, 4800, 800, 1, 398, 1, 4800]))
    cs.append(("held_l1r1s2", 25, 10, 1, 1, 2, avoid_assert(400, 160, 1, [100, 199, 100, 161, 4800, 79, 1, 4800])))
    # fewer than 2 r frames in a push: r = 2, three frames (rem 320 + 500 = 820) -- the next push's windows start late
    cs.append(("short_fr_l2r2s3", 25, 10, 2, 2, 3, [4800, 500, 4800, 480, 481, 4800, 4800]))
    cs.append(("short_fr_l2r2s1", 25, 10, 2, 2, 1, [4800, 500, 4800, 480, 481, 4800]))
    # the r = 1 assertion: one frame for a right context of one (first push; after a steady push)
    cs.append(("assert_first_l1r1s2", 25, 10, 1, 1, 2, [450]))
    cs.append(("assert_later_l1r1s2", 25, 10, 1, 1, 2, [4800, 4800, 100]))
    cs.append(("assert_later_l1r1s1", 25, 10, 1, 1, 1, [1000, 0, 120, 1, 95]))
    # frame shift != 160: 20 ms / 5 ms frames (320 / 80 samples)
    cs.append(("shift80_l0r0s2", 20, 5, 0, 0, 2, random_sizes(rng, 12000, 2000)))
    cs.append(("shift80_l2r2s3", 20, 5, 2, 2, 3, random_sizes(rng, 12000, 2000)))
    return cs


def main():
    skc = load_reference()
    rng = np.random.default_rng(20261018)
    arrays = {}
    names = []
    for name, L_ms, S_ms, left, right, skip, pushes in cases(rng):
        L, S = L_ms * RATE // 1000, S_ms * RATE // 1000
        assert sum(pushes) < 32768, name          # the ramp stays inside int16
        kws = make_spotter(skc, L_ms, S_ms, left, right, skip)
        W = left + right + 1
        kinds, counts, mats, done, at = [], [], [], [], 0
        for n in pushes:
            wave = b"".join(struct.pack("<h", g) for g in range(at, at + n))
            at += n
            done.append(n)
            try:
                res = kws.accept_wave(wave)
            except AssertionError:
                kinds.append(-2)
                counts.append([-1, -1, -1])       # (the reference has already cut its leftover: the library changes nothing)
                break
            if res is None:
                kinds.append(-1)
            else:
                m = res.numpy()
                assert m.shape[1] == W * 4 and np.array_equal(m, np.round(m)), name
                kinds.append(m.shape[0])
                mats.append(m.astype(np.int32))
            fr = -1 if kws.feature_remained is None else int(kws.feature_remained.shape[0])
            counts.append([int(kws.wave_remained.size), fr, int(kws.feats_ctx_offset)])
        arrays[f"cfg/{name}"] = np.array([L, S, left, right, skip], np.int32)
        arrays[f"n/{name}"] = np.array(done, np.int32)
        arrays[f"kind/{name}"] = np.array(kinds, np.int32)
        arrays[f"counts/{name}"] = np.array(counts, np.int32).reshape(len(kinds), 3)
        arrays[f"rows/{name}"] = np.concatenate(mats + [np.zeros((0, W * 4), np.int32)])
        names.append(name)
    arrays["names"] = np.array(names)
    path = os.path.join(HERE, "stream_frontend_golden.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes;", len(names), "cases;",
          sum(int(arrays[f"n/{n}"].size) for n in names), "pushes")


if __name__ == "__main__":
    main()
