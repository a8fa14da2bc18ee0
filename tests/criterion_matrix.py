"""Case list and bars of the criterion tests (tests/test_criterion_oracle.py on the CPU, tests/test_hip_criterion.py on the
GPU; goldens: tests/golden/make_criterion_golden.py -> criterion_golden.npz from the live wekws.model.loss.criterion).

Cases are the smallest shapes at which a kernel can still go wrong: more rows than one workgroup holds (300 = 75 workgroups
of four waves), K that does and does not divide the wave, T = 1, lengths 0 / 1 / T, a vocabulary (2599) that is no multiple of
4 or of 64, 65 and 257 extended CTC states (across a wave, across a workgroup of 256), adjacent repeated labels, an
infeasible row, NaNs in valid and in masked frames, a score of exactly 0.5.  In every max-pooling case the longest
utterance fills the batch: the reference fails otherwise.

Inputs of at most SMALL elements are stored in the golden file; larger ones (V = 2599) are regenerated here from the case's
numpy Generator seed, and the golden file keeps a float64 checksum of them.

BARS -- unit: u = |got - ref64| / (2^-24 * max(1, |ref64|)) per row, per loss term and for the batch loss, ref64 the float64
oracle (tests/criterion_ref.py) on the same float32 inputs.  Rule: pow2_at_or_above(4 x the worst u of the reference's own
float32 result -- torch on the CPU: the batch loss that criterion() returns and the per-row values of the same torch calls
with reduction='none' -- over the matrix); 4 because the device works in the same float32 but its exp / log and its
summation order differ from ATen's.  Measured by make_criterion_golden.py (printed there, stored as <kind>/ref_units):

    kind          reference's worst u   bar    device's worst u (MI355X)
    max_pooling   12.07 (mp_300x3x2_md0: the batch loss, 600 terms added in turn)   64     2.64
    ce            4.94  (ce_300x12: the batch mean)                                 32     2.81
    ctc           8.08  (ctc_v40_t300: 257 states, 290 frames)                       64     9.17 (acc_v16_t30)
"""
from __future__ import annotations

import numpy as np

SMALL = 4096
REF_UNITS = {"max_pooling": 12.07, "ce": 4.94, "ctc": 8.08}      # measured: <kind>/ref_units of the golden file (checked on the CPU)
BARS = {"max_pooling": 64.0, "ce": 32.0, "ctc": 64.0}             # pow2_at_or_above(4 x REF_UNITS)


def units(got, ref64):
    """Worst error in the unit of the bars; classes first: a NaN / +-Inf of the oracle must be met exactly."""
    got = np.asarray(got, np.float64).reshape(-1)
    ref = np.asarray(ref64, np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(ref)
    if not (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
            and np.isfinite(got[fin]).all()):
        return float("inf")
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / (2.0 ** -24 * np.maximum(1.0, np.abs(ref[fin])))).max())


# ------------------------------------------------------------------------------------------------ max pooling
# name -> (B, T, K, min_duration, seed)
MAX_POOLING = {
    "mp_5x37x3_md0": (5, 37, 3, 0, 11),
    "mp_5x37x3_md5": (5, 37, 3, 5, 11),
    "mp_5x37x3_md25": (5, 37, 3, 25, 11),      # beyond the length (20) of utterance 2
    "mp_5x37x3_nan": (5, 37, 3, 5, 12),
    "mp_3x1x1": (3, 1, 1, 0, 13),
    "mp_300x3x2_md0": (300, 3, 2, 0, 14),
    "mp_300x3x2_md2": (300, 3, 2, 2, 14),
    "mp_4x9x70": (4, 9, 70, 1, 15),            # more keywords than a wave has lanes
}


def max_pooling_case(name):
    B, T, K, md, seed = MAX_POOLING[name]
    rng = np.random.default_rng(seed)
    s = rng.random((B, T, K), dtype=np.float32)
    if name.startswith("mp_5x37x3"):
        lengths = np.array([37, 1, 20, 0, 37], np.int32)
        target = np.array([0, 1, 2, -1, 3], np.int32)          # each keyword, a filler, an id >= K
        s[0, 7, 0] = 1.25                                       # above the clamp
        s[0, 9, 1] = -0.25
        s[2, :, :] *= 0.4                                       # utterance 2 stays below 0.5 ...
        s[2, 11, 2] = 0.5                                       # ... except for exactly 0.5 in its keyword column
        if name.endswith("_nan"):
            s[0, 3, 1] = np.nan                                 # valid frame, other column
            s[2, 30, 0] = np.nan                                # masked frame (len 20)
            s[4, 2, 2] = np.nan                                 # valid frame
            s[1, 0, 1] = np.nan                                 # valid for the accuracy, masked for the keyword by min_duration
    elif name == "mp_3x1x1":
        s[:, 0, 0] = [0.5, 0.75, 0.25]
        lengths = np.array([1, 1, 1], np.int32)
        target = np.array([-1, 0, -1], np.int32)
    else:
        lengths = rng.integers(0, T + 1, B).astype(np.int32)
        lengths[B // 2] = T
        lengths[0] = 0
        target = rng.integers(-1, K + 1, B).astype(np.int32)
        s[1::7] *= 0.45                                         # utterances that never reach 0.5
    return dict(scores=s, target=target, lengths=lengths, min_duration=md)


# ------------------------------------------------------------------------------------------------ cross entropy
CE = {f"ce_{B}x{D}": (B, D, 100 + i) for i, (B, D) in enumerate((b, d) for d in (2, 12, 2599) for b in (1, 7, 300))}


def ce_case(name):
    B, D, seed = CE[name]
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, D)) * 3).astype(np.float32)
    target = rng.integers(0, D, B).astype(np.int32)
    if B >= 7:
        x[3, D - 1] = x[3].max()                                # a tie of the maximum: first arg-max
        target[3] = int(np.argmax(x[3]))
        target[5] = int(np.argmax(x[5]))                        # at least one more correct row
    return dict(logits=x, target=target)


# ------------------------------------------------------------------------------------------------ ctc
# name -> (V, T, rows of (length, labels), seed)
_REP5 = [3, 3, 2, 2, 2]
CTC = {
    "ctc_v7_t1": (7, 1, [(1, []), (1, [4]), (1, [2, 5])], 201),                               # the last: infeasible
    "ctc_v7_t50": (7, 50, [(50, []), (50, [6]), (50, _REP5), (30, [1, 2, 3, 4, 5]), (12, _REP5), (7, [1, 1, 1, 1, 1]),
                           (8, _REP5), (1, [5]), (9, [1, 1, 1, 1, 1])], 202),                  # row 5: 5 labels + 4 repeats > 7
    "ctc_v2599_t50": (2599, 50, [(50, []), (50, [2598]), (41, [7, 7, 1300, 1300, 64]), (50, [1, 2598, 63, 64, 65])], 203),
    "ctc_v2599_t1": (2599, 1, [(1, []), (1, [1234])], 204),
    "ctc_v40_t300": (40, 300, [(300, "s32"), (290, "s128")], 205),                            # 65 and 257 extended states
}


def ctc_case(name):
    V, T, rows, seed = CTC[name]
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((len(rows), T, V)) * 2).astype(np.float32)
    labs = []
    for _, lab in rows:
        if isinstance(lab, str):
            n = int(lab[1:])
            lab = rng.integers(1, V, n)
            lab[5:9] = lab[5]                                   # adjacent repeats in the long rows too
            lab = lab.tolist()
        labs.append(list(lab))
    Lmax = max(1, max(len(l) for l in labs))
    targets = np.zeros((len(rows), Lmax), np.int32)
    for i, l in enumerate(labs):
        targets[i, :len(l)] = l
    return dict(logits=x, targets=targets, lengths=np.array([r[0] for r in rows], np.int32),
                target_lengths=np.array([len(l) for l in labs], np.int32))


# ------------------------------------------------------------------------------------------------ utterance accuracy
ACC = {"acc_v16_t30": (16, 30, 8, 301)}


def acc_case(name):
    """Peaked posteriors: per frame one class at logit 12 (posterior > 0.99) or two at 12 / 11 (0.73 / 0.27), the rest
    N(0, 0.3) (below 1e-4): every first-beam decision clears the 0.05 filter and its rank ties by a wide margin."""
    V, T, B, seed = ACC[name]
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, V)) * 0.3).astype(np.float32)
    labels = [[3, 3, 7], [5], [], [9, 2, 2, 11], [1, 2, 3, 4, 5, 6], [15, 15], [8, 4], [12]]
    spoken = [[3, 3, 7], [5, 6], [4], [9, 2, 11], [1, 2, 3, 4, 5, 6], [15], [8, 4], []]     # what the frames say
    lengths = np.array([30, 30, 30, 22, 30, 30, 17, 30], np.int32)
    for b in range(B):
        t = 1
        prev = None
        for tok in spoken[b]:
            if tok == prev:
                x[b, t, 0] = 12.0                               # a blank between repeated tokens
                t += 1
            for _ in range(2):
                x[b, t, tok] = 12.0
                t += 1
            prev = tok
        for u in range(T):
            if x[b, u].max() < 6:
                x[b, u, 0] = 12.0                               # blank everywhere else
        if spoken[b]:
            x[b, 2, 0] = 11.0                                   # a second candidate beside the first token's second frame
    Lmax = max(len(l) for l in labels)
    targets = np.zeros((B, Lmax), np.int32)
    for i, l in enumerate(labels):
        targets[i, :len(l)] = l
    return dict(logits=x, targets=targets, lengths=lengths, target_lengths=np.array([len(l) for l in labels], np.int32))


KINDS = {"max_pooling": (MAX_POOLING, max_pooling_case), "ce": (CE, ce_case), "ctc": (CTC, ctc_case), "acc": (ACC, acc_case)}
_INPUT_KEYS = {"max_pooling": "scores", "ce": "logits", "ctc": "logits", "acc": "logits"}


def case_names(kind):
    return sorted(KINDS[kind][0])


def load_case(kind, name, golden=None):
    """The case's inputs: regenerated, and -- where the golden file stores them -- required to equal the stored ones bit
    for bit (the generator's draws are part of the golden)."""
    c = KINDS[kind][1](name)
    if golden is not None:
        big = _INPUT_KEYS[kind]
        for k, v in c.items():
            key = f"{name}/in/{k}"
            if key in golden.files:
                assert np.array_equal(np.asarray(v), golden[key], equal_nan=True), key
            else:
                assert k == big and np.size(v) > SMALL, key
                assert float(golden[f"{name}/in/{k}_sum"]) == float(np.nansum(np.asarray(v, np.float64))), key
    return c
