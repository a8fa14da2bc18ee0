"""CPU: the float64 restatements of tests/augment_ref.py against the reference's own arithmetic typed as processor.py types it,
the recorded bars against what that arithmetic reaches, the draw helpers of wekws_amd.augment against verbatim loops of the
reference on the same random.Random, and the host side of the C ABI (plan numbers, refusals) without a device."""
import ctypes as C
import random

import numpy as np
import pytest

from tests import augment_ref as AR
from wekws_amd import _capi, augment

H = AR.HOP


@pytest.fixture(scope="module")
def cases():
    return AR.reverb_cases()


def test_reverb_restatement_against_scipy_float32_and_the_recorded_bar(cases):
    """signal.convolve of float32 arrays (fft, auto: norm-wise in U; direct: inside the per-sample bound of a float32 sum) agrees
    with the float64 direct sum; the largest fft / auto error is what REVERB_MEASURED records"""
    xs, hs = cases
    worst = 0.0
    for x in xs:
        for h in hs:
            for method in ("fft", "auto"):
                worst = max(worst, AR.reverb_error(AR.reverb_reference_f32(x, h, method), x, h))
            want = AR.reverb(x, h)
            mag = np.convolve(np.abs(x.astype(np.float64)), np.abs(AR.normalised(h)))[:x.size]
            err = np.abs(AR.reverb_reference_f32(x, h, "direct").astype(np.float64) - want)
            assert (err <= (min(len(h), len(x)) + 3) * 2.0 ** -24 * mag + 1e-300).all(), (len(x), len(h))
    print(f"scipy float32 fft / auto: worst {worst:.4f} U (recorded {AR.REVERB_MEASURED})")
    assert 0.5 * AR.REVERB_MEASURED <= worst <= AR.REVERB_MEASURED
    assert AR.K_REVERB == 4.0 * AR.REVERB_MEASURED


def test_fp16_rir_control_misses_the_reverb_bar_on_the_committed_cases(cases):
    xs, hs = cases
    worst = []
    for x in xs:
        for h in hs:
            if len(h) < 64:
                continue
            h16 = AR.normalised(h).astype(np.float16).astype(np.float32)
            got = np.convolve(x.astype(np.float64), h16.astype(np.float64))[:x.size]
            worst.append(AR.reverb_error(got, x, h))
    print(f"fp16 RIR: {min(worst):.1f} .. {max(worst):.1f} U against a bar of {AR.K_REVERB:.2f}")
    assert min(worst) > 10 * AR.K_REVERB


@pytest.mark.parametrize("scale", [1.0, 32768.0])
def test_noise_restatement_against_the_float32_chain_and_the_recorded_bar(scale):
    bank, rows = AR.noise_bank(), AR.noise_rows(scale)
    worst = 0.0
    for x, (n, r, start, snr, _) in zip(rows, AR.NOISE_CASES):
        assert x.size == n
        worst = max(worst, AR.noise_error(AR.add_noise_reference_f32(x, bank[r], start, snr, scale), x, bank[r], start, snr, scale))
    print(f"float32 chain, pcm_scale {scale}: worst {worst:.2f} units (recorded {AR.NOISE_MEASURED})")
    assert 0.5 * AR.NOISE_MEASURED <= worst <= AR.NOISE_MEASURED
    assert AR.K_NOISE == 2.0 * AR.NOISE_MEASURED


def test_noise_segment_is_the_reference_slice_and_resize():
    v = AR.noise(700, 0)
    assert np.array_equal(AR.noise_segment(v, 0, 3000), np.resize(v, (3000,)))
    assert np.array_equal(AR.noise_segment(v, 0, 700), np.resize(v, (700,)))
    assert np.array_equal(AR.noise_segment(v, 100, 500), v[100:600])


def test_floors_decide_silence():
    """a silent utterance is mixed at audio_db = -40, a silent noise adds nothing"""
    v = AR.noise(700, 0)
    out, gv = AR.add_noise(np.zeros(1000), v, 0, 0.0)
    seg = AR.noise_segment(v, 0, 1000).astype(np.float64)
    assert np.allclose(out, np.sqrt(1e-4 / (np.mean(seg ** 2) + 1e-4)) * seg, rtol=1e-12, atol=0)
    x = AR.utterance(1000, 3)
    out, gv = AR.add_noise(x, np.zeros(10), 0, 0.0)
    assert np.array_equal(out, x.astype(np.float64)) and not gv.any()


# ---------------------------------------------------------------------------------------------- draws
KEYS = ["noise-free-sound-0001", "speech-librivox-0002", "music-fma-0003", "babble-0004", "noise-0005"]
NOISE_LENS = [700, 3000, 5000, 16000, 3001]
AUDIO_LENS = [3000, 3000, 700, 5000, 16001, 1, 3001, 2999]            # 3000 / 700 / 5000 / 3001: a noise of exactly that length


@pytest.mark.parametrize("aug_prob", [0.0, 0.5, 1.0])
def test_draw_reverb_makes_the_reference_draws(aug_prob):
    for seed in range(200):
        ours, theirs = random.Random(seed), random.Random(seed)
        got = augment.draw_reverb(ours, 7, aug_prob, 9)
        want = []
        for _ in range(9):                                   # processor.py:377, lmdb_data.py:36
            if aug_prob > theirs.random():
                index = theirs.randint(0, 7 - 1)
                want.append(index)
            else:
                want.append(-1)
        assert got == want and ours.getstate() == theirs.getstate()
    assert aug_prob or set(got) == {-1}


@pytest.mark.parametrize("aug_prob", [0.0, 0.5, 1.0])
def test_draw_noise_makes_the_reference_draws(aug_prob):
    for seed in range(200):
        ours, theirs = random.Random(seed), random.Random(seed)
        which, start, snr = augment.draw_noise(ours, KEYS, NOISE_LENS, AUDIO_LENS, aug_prob)
        for b, audio_len in enumerate(AUDIO_LENS):           # processor.py:399-422
            if aug_prob > theirs.random():
                index = theirs.randint(0, len(KEYS) - 1)
                key = KEYS[index]
                if key.startswith('noise'):
                    snr_range = [0, 15]
                elif key.startswith('speech'):
                    snr_range = [5, 30]
                elif key.startswith('music'):
                    snr_range = [5, 15]
                else:
                    snr_range = [0, 15]
                want_start = 0
                if NOISE_LENS[index] > audio_len:
                    want_start = theirs.randint(0, NOISE_LENS[index] - audio_len)
                noise_snr = theirs.uniform(snr_range[0], snr_range[1])
                assert (which[b], start[b], snr[b]) == (index, want_start, noise_snr)
                assert snr_range[0] <= snr[b] <= snr_range[1]
            else:
                assert which[b] == -1
        assert ours.getstate() == theirs.getstate()
        # what was drawn is a call the library accepts
        lens, ns = np.asarray(NOISE_LENS, np.int32), np.asarray(AUDIO_LENS, np.int32)
        w, s, d = np.asarray(which, np.int32), np.asarray(start, np.int32), np.asarray(snr, np.float64)
        assert _capi.load().wekws_hip_noise_check(lens.ctypes.data, len(lens), len(ns), int(ns.max()), ns.ctypes.data, w.ctypes.data,
                                                  s.ctypes.data, d.ctypes.data, 1.0) == 0, _capi.last_error()


def test_draw_spec_aug_makes_the_reference_draws_and_clips():
    lengths, F = [98, 3, 1, 60, 49], 7                       # masks of up to 50 frames / 10 bins run past T and F
    past_t = past_f = 0
    for seed in range(200):
        ours, theirs = random.Random(seed), random.Random(seed)
        tm, fm = augment.draw_spec_aug(ours, lengths, F)
        assert tm.shape == (5, 2, 2) and fm.shape == (5, 2, 2) and tm.dtype == fm.dtype == np.int32
        for b, max_frames in enumerate(lengths):             # processor.py:228-238
            max_freq = F
            for i in range(2):
                start = theirs.randint(0, max_frames - 1)
                length = theirs.randint(1, 50)
                end = min(max_frames, start + length)
                past_t += start + length > max_frames
                assert tuple(tm[b, i]) == (start, end)
            for i in range(2):
                start = theirs.randint(0, max_freq - 1)
                length = theirs.randint(1, 10)
                end = min(max_freq, start + length)
                past_f += start + length > max_freq
                assert tuple(fm[b, i]) == (start, end)
        assert ours.getstate() == theirs.getstate()
        ns = np.asarray(lengths, np.int32)
        assert _capi.load().wekws_hip_spec_mask(None, 5, 98, F, ns.ctypes.data, tm.ctypes.data, 2, fm.ctypes.data, 2, None, None) != 0
        assert "NULL" in _capi.last_error()                  # (the masks passed the check: the refusal is the missing tensor)
    assert past_t > 100 and past_f > 100
    tm, fm = augment.draw_spec_aug(random.Random(0), lengths, F, num_t_mask=0, num_f_mask=3, max_t=5, max_f=2)
    assert tm.shape == (5, 0, 2) and fm.shape == (5, 3, 2)


def test_spec_aug_restatement_is_the_reference_loop():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 20, 8)).astype(np.float32)
    y = x[0].copy()
    y[3:9, :] = 0; y[18:20, :] = 0; y[:, 2:5] = 0
    assert np.array_equal(AR.spec_aug(x, [[[3, 9], [18, 20]]], [[[2, 5]]])[0], y)
    z = AR.spec_aug(x, [[[3, 9]]], [[[2, 5]]], lengths=[10])[0]
    assert np.array_equal(z[10:], x[0, 10:]) and not z[:10, 2:5].any() and not z[3:9].any()


# ---------------------------------------------------------------------------------------------- the plan, without a device
def plan_restated(L, B, nmax):
    P = -(-L // H)
    blocks = -(-nmax // H)
    spectra = B * blocks * (H + 1) * 8
    return [P, blocks, spectra + -(-B * 4 // 16) * 16, P * (H + 1) * 8]


def test_plan_numbers():
    lib = _capi.load()
    assert lib.wekws_hip_reverb_hop() == H
    out = (C.c_int64 * 4)()
    sizes = [0, 1, 2, H - 1, H, H + 1, 2 * H - 1, 2 * H, 2 * H + 1, 3 * H, 16000, 64000, 2 ** 30 - 1]
    for L in sizes[1:]:
        for nmax in sizes:
            for B in (0, 1, 3, 4, 5, 1024):
                assert lib.wekws_hip_reverb_plan(L, B, nmax, out) == 0, _capi.last_error()
                assert list(out) == plan_restated(L, B, nmax), (L, B, nmax)
    for L, B, nmax in ((0, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (2 ** 30, 1, 1), (1, 1, 2 ** 30)):
        assert lib.wekws_hip_reverb_plan(L, B, nmax, out) == -1
    assert lib.wekws_hip_reverb_plan(1, 1, 1, None) == -1
    assert lib.wekws_hip_reverb_workspace_bytes(None, 1, 1) == 0


def i32(*v):
    return np.asarray(v, dtype=np.int32)


def test_reverb_refusals_on_the_host():
    lib = _capi.load()
    lens = i32(10, 5000)

    def check(B, nmax, nsamp, rir):
        return lib.wekws_hip_reverb_check(lens.ctypes.data, 2, B, nmax, None if nsamp is None else nsamp.ctypes.data, rir.ctypes.data)

    assert check(3, 100, i32(0, 100, 7), i32(-1, 0, 1)) == 0 and check(2, 100, None, i32(1, 1)) == 0
    for nsamp, rir, word in ((i32(0, 101, 7), i32(0, 0, 0), "row 1"), (i32(0, -1, 7), i32(0, 0, 0), "row 1"),
                             (i32(1, 1, 1), i32(0, 0, 2), "row 2"), (i32(1, 1, 1), i32(-2, 0, 0), "row 0")):
        assert check(3, 100, nsamp, rir) == -1 and word in _capi.last_error(), _capi.last_error()
    assert check(-1, 100, None, i32(0)) == -1 and check(1, -1, None, i32(0)) == -1 and check(1, 2 ** 30, None, i32(0)) == -1
    # creation: refused before the device is asked for
    h = C.c_void_p()
    bank = np.zeros((2, 8), dtype=np.float32)
    bank[0, :3] = 1.0
    bank[1, :8] = 2.0
    for name in ("wekws_hip_reverb_create", "wekws_hip_noise_create"):
        create = getattr(lib, name)
        for ln in (i32(3, 0), i32(3, 9), i32(-1, 8)):
            assert create(bank.ctypes.data, ln.ctypes.data, 2, 8, 0, C.byref(h)) == -1 and not h, name
        assert create(None, lens.ctypes.data, 2, 8, 0, C.byref(h)) == -1 and create(bank.ctypes.data, lens.ctypes.data, 0, 8, 0, C.byref(h)) == -1
    for poison in (np.nan, np.inf, -np.inf):
        bad = bank.copy()
        bad[1, 4] = poison
        assert lib.wekws_hip_reverb_create(bad.ctypes.data, i32(3, 8).ctypes.data, 2, 8, 0, C.byref(h)) == -1 and not h
        assert "RIR 1" in _capi.last_error()
        bad[1, 4] = 0.0                                      # (past the length: not part of the RIR)
        bad[0, 5] = poison
        rc = lib.wekws_hip_reverb_create(bad.ctypes.data, i32(3, 8).ctypes.data, 2, 8, 0, C.byref(h))
        assert rc in (0, -3), (rc, _capi.last_error())       # created, or no device to create it on: not refused
        if rc == 0:
            lib.wekws_hip_reverb_destroy(h)
            h = C.c_void_p()
    zero = bank.copy()
    zero[0, :3] = 0.0
    assert lib.wekws_hip_reverb_create(zero.ctypes.data, i32(3, 8).ctypes.data, 2, 8, 0, C.byref(h)) == -1 and "all zeros" in _capi.last_error()
    assert lib.wekws_hip_reverb_apply(None, None, 1, 1, None, None, None, None) == -1 and "NULL" in _capi.last_error()
    lib.wekws_hip_reverb_destroy(None)
    lib.wekws_hip_noise_destroy(None)


def test_noise_refusals_on_the_host():
    lib = _capi.load()
    lens = i32(700, 3000, 5000)

    def check(nsamp, which, start, snr, scale=1.0, B=3, nmax=3000):
        snr = np.asarray(snr, dtype=np.float64)
        return lib.wekws_hip_noise_check(lens.ctypes.data, 3, B, nmax, None if nsamp is None else nsamp.ctypes.data, which.ctypes.data,
                                         start.ctypes.data, snr.ctypes.data, scale)

    ok = (i32(3000, 3000, 2500), i32(0, 1, 2), i32(5000, 77, 2500), [0.0, 5.0, -5.0])
    assert check(*ok) == 0, _capi.last_error()
    assert check(i32(3000, 3000, 2500), i32(-1, -1, -1), i32(-5, -5, -5), [np.nan] * 3) == 0     # (a copied row's draws are not read)
    for nsamp, which, start, snr, word in (
            (ok[0], ok[1], i32(0, 0, 2501), ok[3], "row 2"),             # a longer noise run past its end
            (ok[0], ok[1], i32(-1, 0, 0), ok[3], "row 0"),
            (ok[0], i32(0, 3, 2), ok[2], ok[3], "row 1"),
            (i32(3000, 3001, 2500), ok[1], ok[2], ok[3], "row 1"),
            (ok[0], ok[1], ok[2], [0.0, np.inf, 0.0], "row 1")):
        assert check(nsamp, which, start, snr) == -1 and word in _capi.last_error(), _capi.last_error()
    for scale in (0.0, -1.0, np.nan, np.inf):
        assert check(*ok, scale=scale) == -1 and "pcm_scale" in _capi.last_error()
    assert lib.wekws_hip_noise_mix(None, None, 1, 1, None, None, None, None, 1.0, None, None) == -1


def test_mask_refusals_on_the_host():
    lib = _capi.load()

    def call(lengths, tm, fm, B=2, T=10, F=4):
        tm, fm = np.asarray(tm, dtype=np.int32).reshape(B, -1, 2), np.asarray(fm, dtype=np.int32).reshape(B, -1, 2)
        rc = lib.wekws_hip_spec_mask(None, B, T, F, None if lengths is None else lengths.ctypes.data, tm.ctypes.data if tm.size else None,
                                     tm.shape[1], fm.ctypes.data if fm.size else None, fm.shape[1], None, None)
        return rc, _capi.last_error()

    assert "NULL" in call(None, [[[0, 10]], [[9, 10]]], [[[0, 4]], [[4, 4]]])[1]          # a good call but for the tensors
    assert "NULL" in call(i32(10, 0), [[[0, 10]], [[0, 0]]], [], B=2)[1]
    for lengths, tm, fm, word in ((None, [[[0, 11]], [[0, 1]]], [[[0, 1]], [[0, 1]]], "row 0"),
                                  (i32(10, 5), [[[0, 1]], [[0, 6]]], [[[0, 1]], [[0, 1]]], "row 1"),
                                  (None, [[[0, 1]], [[3, 2]]], [[[0, 1]], [[0, 1]]], "row 1"),
                                  (None, [[[0, 1]], [[0, 1]]], [[[0, 5]], [[0, 1]]], "row 0"),
                                  (None, [[[0, 1]], [[0, 1]]], [[[0, 1]], [[-1, 1]]], "row 1"),
                                  (i32(10, 11), [[[0, 1]], [[0, 1]]], [[[0, 1]], [[0, 1]]], "row 1")):
        rc, msg = call(lengths, tm, fm)
        assert rc == -1 and word in msg and "NULL" not in msg, msg
    assert lib.wekws_hip_spec_mask(None, 0, 10, 4, None, None, 0, None, 0, None, None) == 0
    assert lib.wekws_hip_spec_mask(None, -1, 10, 4, None, None, 0, None, 0, None, None) == -1
