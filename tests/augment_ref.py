"""float64 restatements of the three augmentation stages of wekws/dataset/processor.py -- add_reverb (374-392), add_noise
(395-430), spec_aug (206-240) -- with the bars and the case tables of tests/test_augment_ref.py (CPU) and
tests/test_hip_augment.py (GPU).  numpy only; independent of the library.  (processor.py itself cannot be imported here: it
needs torchaudio and lmdb.)

Bars.  Reverberation: the error of a row is taken norm-wise, in units of U = 2^-24 |h|_2 |x|_2 -- an FFT method's error is
norm-wise, the reference's own FFT path does not meet a per-sample sum |h| |x| bound either.  K_REVERB is 4 times the largest
error, in U, of the reference's own float32 signal.convolve (methods fft and auto) on REVERB_ROWS x REVERB_RIRS against the
float64 oracle: REVERB_MEASURED.  Noise: per sample, in units of 2^-24 (|x| + |g v|); K_NOISE is 2 times the largest error of
the reference's float32 chain, typed as processor.py types it, on NOISE_CASES: NOISE_MEASURED.  tests/test_augment_ref.py
measures both again and holds the recorded values to what it finds."""
import numpy as np

HOP = 2048                                      # wekws_hip_reverb_hop()

REVERB_MEASURED = 0.43                          # largest error of scipy's float32 paths on the cases below, in U
K_REVERB = 4.0 * REVERB_MEASURED
NOISE_MEASURED = 16.2                           # largest error of the reference's float32 chain (numpy >= 2 scalar rules), in units
K_NOISE = 2.0 * NOISE_MEASURED

REVERB_ROWS = (1, HOP - 1, HOP, HOP + 1, 2 * HOP + 1, 3 * HOP)
REVERB_RIRS = (1, 2, HOP - 1, HOP, HOP + 1, 2 * HOP + 1)


# ---------------------------------------------------------------------------------------------- inputs
def utterance(n, seed, scale=1.0):
    """speech-like float32 in [-scale, scale]: a silent lead-in, then noise under a slow envelope"""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(n)
    env = 0.05 + 0.6 * np.abs(np.sin(2 * np.pi * (t + 37.0 * seed) / 1900.0))
    x = np.clip(rng.standard_normal(n) * 0.3 * env, -1.0, 1.0)
    x[:min(n // 8, 300)] = 0.0
    return (x * scale).astype(np.float32)


def rir(L, seed):
    """an RIR as wavfile.read gives it (int16 values as float32): a direct path and an exponentially decaying tail of 60 dB"""
    rng = np.random.default_rng(2000 + seed)
    k = np.arange(L)
    h = 0.35 * rng.standard_normal(L) * np.exp(-6.9 * k / max(L, 2))
    h[0] = 1.0
    return np.round(h * 20000.0).astype(np.float32)


def noise(n, seed, silent=False):
    """a noise as wavfile.read gives it: int16 values as float32"""
    if silent:
        return np.zeros(n, dtype=np.float32)
    rng = np.random.default_rng(3000 + seed)
    return np.round(np.clip(rng.standard_normal(n) * 2500.0, -32768, 32767)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- add_reverb
def normalised(h):
    """processor.py:383-386 in float64: rir_audio / sqrt(sum(rir_audio ** 2)), of the float32 samples"""
    h = np.asarray(h, dtype=np.float32).astype(np.float64)
    return h / np.sqrt(np.sum(h ** 2))


def reverb(x, h):
    """processor.py:387-388 in float64: signal.convolve(audio, rir, 'full')[:len(audio)], as the direct sum"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.convolve(x, normalised(h))[:x.size]


def reverb_unit(x, h):
    """U = 2^-24 |h|_2 |x|_2 with the normalised RIR (|h|_2 = 1)"""
    return 2.0 ** -24 * float(np.sqrt(np.sum(np.asarray(x, dtype=np.float64) ** 2)))


def reverb_error(got, x, h):
    """largest error of a row against the oracle, in U (0 for an all-zero row that comes back all zero)"""
    err = float(np.abs(np.asarray(got, dtype=np.float64) - reverb(x, h)).max())
    u = reverb_unit(x, h)
    return err / u if u > 0 else (0.0 if err == 0 else np.inf)


def reverb_reference_f32(x, h, method):
    """processor.py:383-388 as typed: the float32 RIR normalised in float32, scipy's convolve of float32 arrays"""
    from scipy import signal
    rir_audio = np.asarray(h).astype(np.float32)
    rir_audio = rir_audio / np.sqrt(np.sum(rir_audio ** 2))
    return signal.convolve(np.asarray(x, dtype=np.float32), rir_audio, mode="full", method=method)[:len(x)]


def reverb_cases():
    """every row length with every RIR length: (row index, rir index, x, h)"""
    xs = [utterance(n, i) for i, n in enumerate(REVERB_ROWS)]
    hs = [rir(L, j) for j, L in enumerate(REVERB_RIRS)]
    return xs, hs


# ---------------------------------------------------------------------------------------------- add_noise
def noise_segment(v, start, n):
    """processor.py:416-421: noise[start:start + n] of a longer noise, else np.resize (a cyclic repeat) -- here from `start`"""
    v = np.asarray(v)
    return v[(int(start) + np.arange(n)) % v.size]


def add_noise(pcm, v, start, snr_db, pcm_scale=1.0):
    """processor.py:402, 422-426 in float64 on pcm / pcm_scale; returns (out in pcm's scale, |g v| in pcm's scale)"""
    audio = np.asarray(pcm, dtype=np.float64) / pcm_scale
    seg = noise_segment(v, start, audio.size).astype(np.float64)
    audio_db = 10 * np.log10(np.mean(audio ** 2) + 1e-4)
    noise_db = 10 * np.log10(np.mean(seg ** 2) + 1e-4)
    g = np.sqrt(10 ** ((audio_db - noise_db - snr_db) / 10))
    return (audio + g * seg) * pcm_scale, np.abs(g * seg) * pcm_scale


def add_noise_reference_f32(pcm, v, start, snr_db, pcm_scale=1.0):
    """processor.py:400-426 as typed, on float32 arrays (audio in [-1, 1] scale, the noise in int16 scale)"""
    audio = (np.asarray(pcm, dtype=np.float32) / np.float32(pcm_scale)).astype(np.float32)
    noise_audio = noise_segment(v, start, audio.size).astype(np.float32)
    audio_db = 10 * np.log10(np.mean(audio**2) + 1e-4)
    noise_snr = float(snr_db)
    noise_db = 10 * np.log10(np.mean(noise_audio**2) + 1e-4)
    noise_audio = np.sqrt(10**(
        (audio_db - noise_db - noise_snr) / 10)) * noise_audio
    out_audio = audio + noise_audio
    return out_audio.astype(np.float64) * pcm_scale


def noise_error(got, pcm, v, start, snr_db, pcm_scale=1.0):
    """largest error against the oracle in units of 2^-24 (|x| + |g v|); where the unit is 0 the sample must be exact"""
    want, gv = add_noise(pcm, v, start, snr_db, pcm_scale)
    unit = 2.0 ** -24 * (np.abs(np.asarray(pcm, dtype=np.float64)) + gv)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    if (err[unit == 0] != 0).any():
        return np.inf
    return float((err[unit > 0] / unit[unit > 0]).max()) if (unit > 0).any() else 0.0


NOISE_BANK = (("noise_short", 700, False), ("speech_equal", 3000, False), ("music_long", 5000, False), ("other_silent", 3000, True))
# (samples of the row, noise of the bank, start, snr_db, silent utterance)
NOISE_CASES = ((3000, 0, 123, 0.0, False), (3000, 1, 0, -5.0, False), (3000, 2, 1500, 30.0, False), (2500, 2, 2500, -5.0, False),
               (3000, 2, 1, 0.0, False), (3000, 0, 650, 30.0, True), (3000, 3, 0, 0.0, False), (2999, 1, 0, 0.0, False),
               (1, 0, 699, 0.0, False))


def noise_bank():
    return [noise(n, i, silent) for i, (_, n, silent) in enumerate(NOISE_BANK)]


def noise_rows(pcm_scale=1.0):
    return [np.zeros(n, dtype=np.float32) if silent else utterance(n, 50 + i, pcm_scale) for i, (n, _, _, _, silent) in enumerate(NOISE_CASES)]


# ---------------------------------------------------------------------------------------------- spec_aug
def masks(m, B):
    """(B, count, 2) int32 of nested [start, end) pairs; count may be 0"""
    a = np.asarray(m, dtype=np.int32)
    return a.reshape(B, a.size // (2 * B) if B else 0, 2)


def spec_aug(feats, t_masks, f_masks, lengths=None):
    """processor.py:228-238 with the masks given: y[start:end, :] = 0 per time mask, y[:, start:end] = 0 per frequency mask,
    within every row's own frames; (B, T, F) in, a copy out"""
    y = np.array(feats, copy=True)
    for b in range(y.shape[0]):
        T = y.shape[1] if lengths is None else int(lengths[b])
        for s, e in masks(t_masks, y.shape[0])[b]:
            y[b, :T][s:e, :] = 0
        for s, e in masks(f_masks, y.shape[0])[b]:
            y[b, :T][:, s:e] = 0
    return y
