"""GPU: the HIP fbank kernel (wekws_hip_fbank_compute) against the reference-recorded goldens and the C oracle.
Tolerance (abs, on log-mel values spanning [-16, 26]): the reference's FFT uses a float32 sine table built by
a recurrence (fft.cc:11-35) and is itself up to 2.4e-5 (40 bins) / 1.7e-4 (80 bins: narrow low-frequency filters
on the pre-emphasised spectrum) away from a float64 evaluation of the same pipeline on these inputs (measured in
the build container); the HIP kernel uses exactly-rounded twiddles, so it cannot be closer to the reference than
that.  40 bins: 1e-4 (SURVEY.md appendix C target); 80 bins: 4e-4."""
import os

import numpy as np
import pytest
import torch

from oracle import fbank_oracle
from tests.golden.fbank_cases import FBANK_CASES, fbank_input
from tests.helpers import K_FBANK
from wekws_amd.frontend import Fbank
from wekws_amd.utils import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
TOL80 = 4e-4


@pytest.fixture(scope="module")
def fgolden():
    return np.load(os.path.join(ROOT, "tests", "golden", "fbank_golden.npz"))


@pytest.mark.parametrize("case", FBANK_CASES, ids=[c["name"] for c in FBANK_CASES])
def test_golden(case, fgolden):
    pcm = fbank_input(case)
    fb = Fbank(num_bins=case["num_bins"], sample_rate=case["sample_rate"])   # (8 / 4 kHz: the reference's 256- / 128-point cases)
    got = fb(torch.from_numpy(pcm).cuda()).cpu().numpy()
    ref = fgolden[case["name"]]
    assert got.shape == ref.shape
    assert float(np.abs(got - ref).max()) <= (TOL80 if case["num_bins"] == 80 else TOL)


def test_batch_1024_vs_oracle_sample():
    pcm = synth.synth_pcm(1024, 16000, seed=9, kind="noise")
    fb = Fbank(40)
    got = fb(torch.from_numpy(pcm).cuda()).cpu().numpy()
    assert got.shape == (1024, 98, 40) and np.isfinite(got).all()
    for i in (0, 1, 511, 1023):
        assert float(np.abs(got[i] - fbank_oracle.fbank(pcm[i], 40)).max()) <= TOL
    # shift property: frame t of the signal delayed by one hop == frame t+1 of the original
    sh = fb(torch.from_numpy(np.ascontiguousarray(pcm[:4, 160:])).cuda()).cpu().numpy()
    assert float(np.abs(sh[:, :97] - got[:4, 1:98]).max()) <= 1e-5


@pytest.mark.parametrize("bins", [40, 80])
def test_deterministic_under_load(bins):
    """The hand-scheduled packed instructions of the kernel (round 6) carry their own wait states: every frame of a full-device
    batch must come back bit-identical on every repeat and in any batch composition (another wave / workgroup assignment)."""
    B = 2048
    pcm = torch.from_numpy(synth.synth_pcm(B, 16000, seed=3, kind="noise")).cuda()
    fb = Fbank(bins)
    first = fb(pcm).clone()
    for _ in range(10):
        assert torch.equal(fb(pcm).view(torch.int32), first.view(torch.int32))
    small = torch.cat([fb(pcm[i:i + 8]).clone() for i in range(0, 512, 8)])
    assert torch.equal(small.view(torch.int32), first[:512].view(torch.int32))
    sample = first[::97].cpu().numpy()
    for k, i in enumerate(range(0, B, 97)):
        if k % 5 == 0:
            ref = fbank_oracle.fbank(pcm[i].cpu().numpy(), bins)
            assert float(np.abs(sample[k] - ref).max()) <= (TOL80 if bins == 80 else TOL)


def test_bit_identical_beside_a_model_forward_on_another_stream():
    """The tenant case of pk_safe.hip.h: the fbank kernel issues no MFMA itself, but a model forward on ANOTHER stream puts MFMA waves
    on its SIMDs -- which is all the gfx950 packed-f32 hazard needs.  A batch small enough to leave room beside an MDTC forward that
    half-fills the CUs, 40 overlapping rounds: every frame bit-identical to the solo run.  (The first cut of this round's hand-written
    butterflies used the op_sel:[0,1] forms and fails this test -- checked with a variant build.)"""
    from tests.test_hip_parity import build
    from wekws_amd import pack
    cfg = dict(synth.MODEL_CONFIGS["mdtc_h64"])
    model = build(cfg, synth.synth_state_dict(pack.model_spec(cfg), 11))
    x = torch.from_numpy(synth.synth_feats(512, 98, cfg["input_dim"], seed=4)).cuda()
    pcm = torch.from_numpy(synth.synth_pcm(768, 16000, seed=5, kind="noise")).cuda()
    fb = Fbank(40)
    ref = fb(pcm).clone()
    y0, _ = model(x)
    y0 = y0.clone()
    torch.cuda.synchronize()
    s_fb, s_md = torch.cuda.Stream(), torch.cuda.Stream()
    bad = 0
    for _ in range(40):
        with torch.cuda.stream(s_md):
            for _ in range(6):
                y, _c = model(x)
        with torch.cuda.stream(s_fb):
            got = [fb(pcm) for _ in range(4)]
        torch.cuda.synchronize()
        bad += sum(int((g.view(torch.int32) != ref.view(torch.int32)).any(dim=-1).sum().item()) for g in got)
        assert torch.equal(y.view(torch.int32), y0.view(torch.int32))
    assert bad == 0, f"{bad} frames differ from the solo run"


def test_short_and_empty():
    fb = Fbank(40)
    assert fb(torch.zeros(2, 399, device="cuda")).shape == (2, 0, 40)
    assert fb(torch.zeros(0, 16000, device="cuda")).shape == (0, 98, 40)
    with pytest.raises(ValueError):
        fb(torch.zeros(2, 16000))


def test_int16_input_equals_widened_float_input():
    """wekws_hip_fbank_compute_i16 (int16 PCM, widened in registers) == wekws_hip_fbank_compute on the same samples as
    float32, bit for bit -- including an odd sample count (unpaired loads) and the full int16 range."""
    fb = Fbank(40)
    for n, kind in ((16000, "noise"), (16000 + 97, "noise"), (16000, "ramp")):
        pcm = synth.synth_pcm(3, n, seed=7, kind=kind)
        i16 = np.clip(np.round(pcm), -32768, 32767).astype(np.int16)
        a = fb(torch.from_numpy(i16.astype(np.float32)).cuda()).cpu().numpy()
        b = fb(torch.from_numpy(i16).cuda()).cpu().numpy()
        assert a.shape == b.shape and np.array_equal(a, b)


def test_very_short_frames_are_refused():
    """Frames of 65 .. 512 samples are served (the reference's 128- / 256- / 512-point FFT cases: the golden cases above
    include 8 kHz and 4 kHz audio); 64 samples or fewer have no recipe and no mel-slot layout: the library says so instead
    of computing other features."""
    from wekws_amd import _capi
    with pytest.raises(_capi.HipLibraryError, match="65 .. 512"):
        Fbank(23, sample_rate=2000)          # 25 ms at 2 kHz = 50 samples
    with pytest.raises(_capi.HipLibraryError):
        Fbank(40, frame_length=600)


def test_80_bin_tolerance_end_to_end(error_report):
    """VERDICT r2 (weak #3): the 80-bin features are held to 4e-4 against the reference front-end instead of appendix C's
    1e-4 (the reference's own float32 recurrence twiddles are 1.7e-4 away from a float64 evaluation).  What that does to
    the POSTERIORS: PCM -> HIP fbank(80) -> HIP MDTC-80d, against C restatement of the reference front-end (bit-exact with
    the compiled reference, tests/test_fbank_oracle.py) -> numpy oracle of the model.  The difference must stay inside the
    posterior bar (1e-4); the measured value goes to parity_errors.json."""
    from oracle import kws_oracle
    from wekws_amd import pack
    from wekws_amd.model.kws_model import init_model
    cfg = dict(synth.MODEL_CONFIGS["mdtc_h64_80d"])
    sd = synth.synth_state_dict(pack.model_spec(cfg), 1234)
    m = init_model(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda().eval()
    worst_f, worst_y = 0.0, 0.0
    for kind, seed in (("noise", 3), ("ramp", 4), ("sine", 5)):
        pcm = synth.synth_pcm(4, 16000, seed=seed, kind=kind)
        feats = Fbank(80)(torch.from_numpy(pcm).cuda())
        y, _ = m(feats)
        ref_feats = np.stack([fbank_oracle.fbank(pcm[i], 80) for i in range(pcm.shape[0])]).astype(np.float32)
        ry, _ = kws_oracle.forward(cfg, sd, ref_feats, None)
        worst_f = max(worst_f, float(np.abs(feats.cpu().numpy() - ref_feats).max()))
        worst_y = max(worst_y, float(np.abs(y.cpu().numpy() - ry).max()))
    error_report["fbank80_end_to_end/features"] = worst_f
    error_report["fbank80_end_to_end/posteriors"] = worst_y
    assert worst_f <= TOL80 and worst_y <= 1e-4, (worst_f, worst_y)


def framing_cases(seed):
    """The seeded configurations of test_random_framings_against_the_c_oracle (also walked by tools/probe/fbank_fuzz_diag.py)."""
    rng = np.random.default_rng(4200 + seed)
    for trial in range(10):
        sr = int(rng.choice([16000, 16000, 8000, 4000]))
        flen = int(rng.choice([sr // 1000 * 25, int(rng.integers(65, 513))]))
        shift = int(rng.choice([sr // 1000 * 10, int(rng.integers(1, 400))]))
        bins = int(rng.choice([40, 80, 23, 64, 128]))
        window = str(rng.choice(["hamming", "povey"]))
        B = int(rng.choice([1, 3, 17]))
        nf = int(rng.integers(0, 40))
        nsamp = max(0, flen + (nf - 1) * shift + int(rng.integers(0, shift))) if nf else int(rng.integers(0, flen))
        kind = str(rng.choice(["noise", "sine"]))
        pcm = synth.synth_pcm(B, max(nsamp, 1), seed=trial, kind=kind)[:, :nsamp]
        yield (seed, trial, sr, flen, shift, bins, window, B, nsamp, kind), pcm


def framing_bound(ref, tol):
    """Allowed |got - ref| per bin: the module's tolerance plus float32's resolution of the frame's PEAK amplitude as seen from the
    bin -- 4 eps exp((peak - ref) / 2) in log energy (a bin 60 dB below the frame's peak holds 1/1000 of its amplitude: one part in
    2^23 of the peak is 1.2e-4 of the bin).  Both extractors are float32 pipelines with different FFTs (the reference: radix-2,
    recurrence twiddles, fft.cc:11-119; the kernel: radix-4, exactly rounded twiddles), so that is how close they can be; measured
    over 2,300 seeds = 121,480 utterances (tools/probe/fuzz_all.py, profiles/r06_experiments.txt): the factor needed is <= 1.64."""
    eps = float(np.finfo(np.float32).eps)
    return tol + 4.0 * eps * np.exp((ref.max(axis=-1, keepdims=True) - ref).astype(np.float64) / 2)


@pytest.mark.parametrize("seed", [0, 1, 2, 558, 917, 2175, 2208, 2221, 2235])
def test_random_framings_against_the_c_oracle(seed, error_report):
    """Seeded fuzz of the extractor's configuration space (fbank.h:33-97 takes any bin count / frame length; feature_pipeline.cc
    any sample count): random sample rates, frame lengths 65 .. 512, shifts, bin counts, windows, batch sizes and lengths around
    the framing boundaries, float and int16 input, against the plain-C oracle (bit-exact against the compiled reference front-end,
    tests/test_fbank_oracle.py), every bin within framing_bound.  Seeds >= 558: the configurations of a 2,300-seed run that come
    closest to the bound (pure tones through short FFTs; 558 and 917 are the worst at <= 40 / > 40 bins).
    Every bin is also held to the float64 evaluation fbank_f64 in fbank_units at K_FBANK."""
    worst = 0.0
    for what, pcm in framing_cases(seed):
        _, trial, sr, flen, shift, bins, window, B, nsamp, kind = what
        if fbank_oracle.has_empty_filter(bins, sr, flen):   # the reference's constructor CHECK-fails (fbank.h:81): refused, not wrong
            with pytest.raises(Exception, match="covers no FFT bin"):
                Fbank(num_bins=bins, sample_rate=sr, frame_length=flen, frame_shift=shift, window=window)
            continue
        fb = Fbank(num_bins=bins, sample_rate=sr, frame_length=flen, frame_shift=shift, window=window)
        got = fb(torch.from_numpy(np.ascontiguousarray(pcm)).cuda()).cpu().numpy()
        assert got.shape == (B, fbank_oracle.num_frames(nsamp, flen, shift), bins), what
        tol = TOL if bins <= 40 else TOL80
        for i in range(B):
            ref = fbank_oracle.fbank(pcm[i], bins, sr, flen, shift, 0 if window == "hamming" else 1)
            assert got[i].shape == ref.shape, (what, i)
            if ref.size:
                over = np.abs(got[i] - ref) - framing_bound(ref, tol)
                assert float(over.max()) <= 0.0, (what, i, float(over.max()), float(np.abs(got[i] - ref).max()))
                # ... and every bin against the float64 evaluation at the tight bar (tests/helpers.py::K_FBANK)
                u = fbank_oracle.fbank_units(got[i], pcm[i], bins, sr, flen, shift, 0 if window == "hamming" else 1)
                worst = max(worst, float(u.max()))
                assert float(u.max()) <= K_FBANK, (what, i, float(u.max()), np.unravel_index(int(u.argmax()), u.shape))
        if nsamp:
            i16 = torch.from_numpy(np.ascontiguousarray(pcm).astype(np.int16)).cuda()
            assert torch.equal(fb(i16), fb(i16.float())), what
    error_report[f"fbank_f64/fuzz_seed{seed}"] = worst
