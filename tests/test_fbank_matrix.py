"""CPU: the fbank variant matrix (tests/fbank_matrix.py) against fbank_build_tables, run without a device through the hooks
library's wekws_hip_debug_fbank_plan; the calibration of K_FBANK / K_DCT (tests/helpers.py) from the reference side; the CPU
emulation of the negative controls of tests/test_hip_fbank_f64.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import fbank_oracle, kaldi_feats_oracle as kf
from tests import fbank_matrix as fm
from tests.helpers import CONTROL_MARGIN, K_DCT, K_FBANK, pow2_at_or_above
from tests.test_hip_fbank import framing_cases

# 16 sample rates from 2 to 96 kHz (the usual audio rates: the sweep SAMPLES the rates, it does not take every integer one); every bin
# count 1 .. 128; frame lengths 65 .. 512.  The plan depends on the frame length only through the reference's transform length
# (128 / 256 / 512 points): the edges of the three classes for every rate, every length for three rates.
RATES = (2000, 3000, 4000, 6000, 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 64000, 88200, 96000)
EDGE_LENGTHS = (65, 100, 128, 129, 200, 256, 257, 400, 512)
ALL_LENGTH_RATES = (2000, 16000, 96000)


@pytest.fixture(scope="module")
def hooks():
    return fm.type_hooks(C.CDLL(fm.hooks_path()))


@pytest.mark.parametrize("row", fm.ROWS, ids=[r["id"] for r in fm.ROWS])
def test_rows_name_the_variant_the_tables_give(hooks, row):
    assert fm.row_variant(hooks, row) == row["variant"]
    p = fm.plan(hooks, *fm.row_cfg(row))
    assert (p["fw"], p["waves"]) == (1, 4)            # (what the rows' frame counts and sample_utterances are laid out for)
    assert p["slot_w_off"] + 16 * p["nslots"] == p["table_floats"] and p["slot_bin_off"] == p["slot_first_off"] + p["nslots"]


@pytest.fixture(scope="module")
def sweep(hooks):
    """{(rounds, stride): example}, the largest slot count, {stride: set of transform-length classes seen}."""
    reach, most = {}, (0, None)
    for sr in RATES:
        for flen in (range(65, 513) if sr in ALL_LENGTH_RATES else EDGE_LENGTHS):
            for bins in range(1, 129):
                p = fm.plan(hooks, bins, sr, flen)
                if p["empty"] >= 0:
                    continue
                assert p["stride"] == (4 if flen <= 128 else 2 if flen <= 256 else 1)
                assert p["rounds"] == (p["nslots"] + 63) // 64 and p["nslots"] >= bins
                reach.setdefault((p["rounds"], p["stride"]), (sr, flen, bins))
                if p["nslots"] > most[0]:
                    most = (p["nslots"], (sr, flen, bins))
    return reach, most


def test_three_slot_rounds_are_unreachable(sweep):
    """fbank_kernel<3, S> serves 129 .. 192 slots.  No configuration of the sweep (RATES: sampled rates) that wekws_hip_fbank_create
    accepts has them: a bank of up to 128
    filters without an empty one never needs more than 128 slots (the wide filters that need two or more slots belong to banks of
    few bins).  fbank.hip.h marks the instantiations unreachable; this is the assertion behind the mark."""
    reach, most = sweep
    assert most[0] == 128, most
    assert {r for r, _ in reach} == {1, 2}


def test_every_reachable_variant_has_a_row(sweep):
    reach, _ = sweep
    assert set(reach) == {(r, s) for r in (1, 2) for s in (1, 2, 4)}, reach
    want = {(r, s, p, d) for (r, s) in reach for p in (0, 1) for d in ("f32", "i16")}    # the loads and the sample type are the caller's
    have = {fm.variant_tuple(r["variant"]) for r in fm.ROWS}
    assert want <= have, sorted(want - have)
    slots = {int(r["variant"].split()[-1][5:]) for r in fm.ROWS}
    assert {1, 2, 3, 4} <= slots
    assert {r["flen"] for r in fm.ROWS} >= {65, 128, 129, 256, 257, 400, 512}
    assert {r["bins"] for r in fm.ROWS} >= {23, 40, 64, 80, 126} and {r["window"] for r in fm.ROWS} == set(fm.WINDOWS)
    assert {r["nframes"] for r in fm.ROWS if r["B"] > 1} >= {1, 2}
    assert {r["grid"][0] for r in fm.ROWS if r["grid"]} == {"over", "under"}
    # the three ways out of the paired loads
    single = [r for r in fm.ROWS if " single " in r["variant"]]
    assert any(r["nsamp"] % 2 for r in single) and any(r["shift"] % 2 for r in single)
    assert any(r["x_off"] == 1 and r["dtype"] == "f32" and not (r["nsamp"] % 2 or r["shift"] % 2 or r["flen"] % 2) for r in single)


def test_the_most_bins_a_framing_carries(hooks):
    assert fm.plan(hooks, 126, 16000, 400)["empty"] < 0 <= fm.plan(hooks, 127, 16000, 400)["empty"]
    assert fm.plan(hooks, 66, 4000, 100)["empty"] < 0 <= fm.plan(hooks, 67, 4000, 100)["empty"]
    for bins, sr, flen in ((126, 16000, 400), (127, 16000, 400), (66, 4000, 100), (67, 4000, 100), (128, 8000, 400)):
        assert fbank_oracle.has_empty_filter(bins, sr, flen) == (fm.plan(hooks, bins, sr, flen)["empty"] >= 0)


def test_oracle_bank_is_the_kernel_bank(hooks):
    """The float64 oracle takes its mel weights from the C restatement (libm's logf, like the host code that builds the kernel's
    table).  Here, without a device: both banks have the same supports (the table's weight count is the sum of the oracle's filter
    spans).  The weights themselves are compared bit for bit on the GPU, through the table hook (tests/test_hip_fbank_f64.py)."""
    for bins, sr, flen in ((80, 16000, 400), (40, 8000, 200), (66, 4000, 100), (23, 16000, 65)):
        W = fbank_oracle.mel_bank(bins, sr, flen)
        p = fm.plan(hooks, bins, sr, flen)
        assert p["mel_w_count"] == sum((np.flatnonzero(W[b])[-1] - np.flatnonzero(W[b])[0]) * p["stride"] + 1 for b in range(bins))
    # numpy's float32 log is NOT that function: a bank built with it differs in the last bits of the mel values, tens of eps in a weight
    a, d = fbank_oracle.mel_bank(80, 16000, 400), fbank_oracle.mel_bank(80, 16000, 400, double=True)
    assert 1e-6 < float(np.abs(a - d).max()) < 1e-4


def _units(row_or_cfg, x, **kw):
    cfg = fm.row_cfg(row_or_cfg) if isinstance(row_or_cfg, dict) else row_or_cfg
    return np.stack([fbank_oracle.fbank_units(fbank_oracle.fbank_f32_exact(x[i], *cfg, **kw), x[i], *cfg) for i in range(x.shape[0])])


def _row_batch(row):
    return fm.row_input(row, 8 if row["grid"] else row["B"])


@pytest.fixture(scope="module")
def calibration():
    """The largest fbank_units figure of the plain float32 restatement (and of the reference algorithm) over every row and the first
    utterance of every case of framing_cases(0 .. 39)."""
    exact, ref, silence = (0.0, None), (0.0, None), 0.0
    for row in fm.ROWS:
        x = _row_batch(row)
        u = _units(row, x)
        silence = max(silence, float(u[3::4].max()))
        exact = max(exact, (float(u.max()), row["id"]))
        r = max(float(fbank_oracle.fbank_units(fbank_oracle.fbank(x[i], *fm.row_cfg(row)), x[i], *fm.row_cfg(row)).max()) for i in range(x.shape[0]))
        ref = max(ref, (r, row["id"]))
    for seed in range(40):
        for what, pcm in framing_cases(seed):
            _, trial, sr, flen, shift, bins, window, B, nsamp, kind = what
            cfg = (bins, sr, flen, shift, fm.WINDOWS.index(window))
            if fbank_oracle.has_empty_filter(bins, sr, flen) or not fbank_oracle.num_frames(nsamp, flen, shift):
                continue
            exact = max(exact, (float(_units(cfg, pcm[:1]).max()), what))
            ref = max(ref, (float(fbank_oracle.fbank_units(fbank_oracle.fbank(pcm[0], *cfg), pcm[0], *cfg).max()), what))
    return exact, ref, silence


def test_k_fbank_is_twice_the_float32_restatement(calibration):
    """K_FBANK is the smallest power of two at or above twice what a plain float32 pipeline with exactly rounded twiddles reaches --
    the reference side's arithmetic, not the kernel's.  The reference ALGORITHM itself (recurrence twiddles, radix-2, serial sums)
    stays inside the same bar once the arbiter uses the reference's own mel bank."""
    (exact, where), (ref, ref_where), silence = calibration
    print(f"fbank_f32_exact max u = {exact:.3f} at {where}; reference algorithm {ref:.3f} at {ref_where}; silence {silence:.3f}")
    assert K_FBANK == pow2_at_or_above(2.0 * exact), (exact, where)
    assert exact <= K_FBANK and ref <= K_FBANK, (exact, where, ref, ref_where)
    assert 0.0 < silence <= K_FBANK                   # silence compares at the floor through the same formula


@pytest.mark.parametrize("rid", fm.CONTROL_ROWS)
def test_control_emulations(rid):
    """What the perturbed device tables of tests/test_hip_fbank_f64.py do to a float32 pipeline on the CPU: a mel weight off by 2^-12
    (in its bin alone), the bank computed in double, twiddles on a 2^-18 grid miss the bar by CONTROL_MARGIN at least; twiddles by
    the reference's float32 recurrence (1.5 ulp of 1 off at worst) do NOT -- they are as good as exactly rounded ones, in this unit
    and for the features."""
    row = next(r for r in fm.ROWS if r["id"] == rid)
    assert row["controls"] == fm.CONTROLS
    x = fm.row_input(row)
    b = row["bins"] // 2
    w = _units(row, x, weight=(b, 1.0 + 2.0 ** -12)).max(axis=(0, 1))
    u = {name: float(_units(row, x, **kw).max()) for name, kw in fm.CONTROL_EMULATION.items()}
    print(rid, u, float(w[b]), float(np.delete(w, b).max()))
    assert w[b] >= CONTROL_MARGIN * K_FBANK and np.delete(w, b).max() <= K_FBANK
    assert u["mel_double"] >= CONTROL_MARGIN * K_FBANK and u["coarse_twiddle"] >= CONTROL_MARGIN * K_FBANK
    assert u["twiddle"] <= K_FBANK
    t = fbank_oracle.recurrence_twiddles(512, 256).astype(np.float64) - fbank_oracle.exact_twiddles(512, 256)
    assert 0.0 < float(np.abs(t).max()) <= 2.0 ** -22


def test_two_float64_restatements_of_the_povey_fbank():
    """fbank_f64(window=1) follows the runtime's construction (float32 mel bank, the window rounded to float32, the constant 0.97f);
    kaldi_feats_oracle.fbank follows torchaudio's (everything in double).  They do NOT agree to float32 rounding: 1.23e-4 in the
    log domain (noise, 80 bins, mel bin 2: a narrow low filter on the pre-emphasised spectrum, where the frame's energy cancels).
    Measured stage by stage on that input: 0.97 instead of 0.97f leaves 1.06e-4, the unrounded window 4.3e-5, torchaudio's double
    bank 9.5e-7 -- the float32 rounding of kaldi_feats_oracle's result.  The three are differences of the two PIPELINES' tables,
    not of the arithmetic, so each kernel path is held to its own construction: the fbank kernel to fbank_f64."""
    from wekws_amd.utils import synth
    worst = 0.0
    for kind in ("noise", "sine"):
        for bins in (40, 80):
            pcm = synth.synth_pcm(1, 16000, seed=3, kind=kind)[0]
            worst = max(worst, float(np.abs(fbank_oracle.fbank_f64(pcm, bins, window=1) - kf.fbank(pcm, bins).astype(np.float64)).max()))
    print("fbank_f64(povey) vs kaldi_feats_oracle.fbank:", worst)
    assert 2e-5 < worst <= 2e-4


def test_k_dct_is_twice_a_float32_evaluation():
    worst, control = 0.0, np.inf
    for rows, nb, nc, q in fm.DCT_SHAPES:
        x = fm.dct_input(rows, nb)
        ref, s = kf.dct_lifter(x, nc, q, dtype=np.float64), kf.dct_lifter_scale(x, nc, q)
        worst = max(worst, float((np.abs(kf.dct_lifter_f32(x, nc, q) - ref) / s).max()))
        if nb >= 16 and rows >= 3:                     # one matrix entry x (1 + 2^-12), the largest of a column: that column misses
            # (the kernel computes its matrix itself, there is no table to perturb on the device: a CPU emulation alone.  One row
            # can hide one entry -- its x_j may be small --, so the control is read over three rows or more.)
            k = nc // 2
            j = int(np.argmax(np.abs(kf.dct_matrix(nc, nb)[:, k])))
            e = np.abs(kf.dct_lifter_f32(x, nc, q, entry=(j, k, 1.0 + 2.0 ** -12)) - ref) / s
            control = min(control, float(e[:, k].max()))
    print("dct_lifter float32 max u =", worst, "; least visible perturbed entry", control)
    assert K_DCT == pow2_at_or_above(2.0 * worst) and control >= CONTROL_MARGIN * K_DCT
