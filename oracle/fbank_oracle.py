"""ctypes access to the fbank oracles  --  TEST INFRASTRUCTURE, NOT PRODUCT (see oracle/fbank_oracle.c).

fbank(wave, num_bins)      the plain-C restatement (oracle/_build/libfbank_oracle.so)
ref_fbank(wave, num_bins)  the reference's own C++ front-end compiled into oracle/_ref/ (None if absent)
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PORT = os.path.join(_HERE, "_build", "libfbank_oracle.so")
_REF = os.path.join(_HERE, "_ref", "libref_fbank.so")
_port = _ref = None


def _load_port():
    global _port
    if _port is None:
        if not os.path.exists(_PORT):
            raise RuntimeError(f"{_PORT} missing: run `make -C oracle`")
        _port = C.CDLL(_PORT)
        _port.wekws_oracle_fbank.restype = C.c_int
        _port.wekws_oracle_fbank.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _port.wekws_oracle_mel_bank.restype = C.c_int
        _port.wekws_oracle_mel_bank.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    return _port


def have_ref() -> bool:
    return os.path.exists(_REF)


def num_frames(nsamp, frame_length=400, frame_shift=160):
    return 0 if nsamp < frame_length else 1 + (nsamp - frame_length) // frame_shift


def fbank(wave, num_bins=40, sample_rate=16000, frame_length=400, frame_shift=160, window=0):
    wave = np.ascontiguousarray(wave, dtype=np.float32)
    nf = num_frames(wave.size, frame_length, frame_shift)
    out = np.empty((nf, num_bins), np.float32)
    if nf:
        n = _load_port().wekws_oracle_fbank(wave.ctypes.data, wave.size, num_bins, sample_rate, frame_length,
                                            frame_shift, window, out.ctypes.data)
        assert n == nf
    return out


def ref_fbank(wave, num_bins=40, sample_rate=16000, first_push=0):
    """Reference front-end (25 ms / 10 ms framing fixed by FeaturePipelineConfig, feature_pipeline.h:34-39)."""
    global _ref
    if not have_ref():
        return None
    if _ref is None:
        _ref = C.CDLL(_REF)
        _ref.ref_fbank.restype = C.c_int
        _ref.ref_fbank.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    wave = np.ascontiguousarray(wave, dtype=np.float32)
    nf = num_frames(wave.size, sample_rate // 1000 * 25, sample_rate // 1000 * 10)
    out = np.empty((nf, num_bins), np.float32)
    n = _ref.ref_fbank(wave.ctypes.data, wave.size, num_bins, sample_rate, first_push, out.ctypes.data)
    assert n == nf, (n, nf)
    return out


def has_empty_filter(num_bins=40, sample_rate=16000, frame_length=400):
    """Does a triangular filter of this bank cover no FFT bin?  The reference's constructor CHECK-fails then (fbank.h:51-81), and
    wekws_hip_fbank_create refuses the configuration.  Decided by the C restatement's bank (float32 arithmetic, libm's logf, like
    the reference and like the host code of the kernel's table -- numpy's float32 log is another function in the last bit)."""
    n = 1
    while n < frame_length:
        n *= 2
    W = np.zeros((num_bins, n // 2), np.float32)
    return _load_port().wekws_oracle_mel_bank(num_bins, sample_rate, frame_length, W.ctypes.data) > 0


def mel_bank(num_bins, sample_rate, frame_length, double=False):
    """(num_bins, n / 2) float32 triangular weights, n the padded frame length.  The reference's bank: float32 arithmetic with
    libm's logf, taken from the C restatement (numpy's float32 log is another function -- it differs from logf in the last bit
    for about one argument in eight, and one ulp of a mel value moves a weight by tens of float32 eps).  double=True: the same
    formulas in float64, rounded to float32 at the end (a negative control of the tight bar)."""
    n = 1
    while n < frame_length:
        n *= 2
    nb = n // 2
    W = np.zeros((num_bins, nb), np.float32)
    if not double:
        _load_port().wekws_oracle_mel_bank(num_bins, sample_rate, frame_length, W.ctypes.data)
        return W
    mel = lambda f: 1127.0 * np.log(1.0 + np.float64(f) / 700.0)         # noqa: E731
    lo, hi = mel(20.0), mel(sample_rate // 2)
    delta = (hi - lo) / (num_bins + 1)
    m = mel(sample_rate / n * np.arange(nb))
    for b in range(num_bins):
        left, center, right = lo + b * delta, lo + (b + 1) * delta, lo + (b + 2) * delta
        inside = (m > left) & (m < right)
        W[b] = np.where(inside, np.where(m <= center, (m - left) / (center - left), (right - m) / (right - center)), 0.0)
    return W


def _tables(num_bins, sample_rate, frame_length, window, double_mel=False):
    """(padded length n, mel weights (num_bins, n / 2), window (frame_length,)) as the reference builds them: mel_bank, and the
    window in double rounded to float32."""
    W = mel_bank(num_bins, sample_rate, frame_length, double_mel)
    n = 2 * W.shape[1]
    a = 2.0 * np.pi / (frame_length - 1)
    i = np.arange(frame_length, dtype=np.float64)
    win = (0.54 - 0.46 * np.cos(a * i)) if window == 0 else np.power(0.5 - 0.5 * np.cos(a * i), 0.85)
    return n, W, win.astype(np.float32)


def _frames(wave, frame_length, frame_shift):
    wave = np.ascontiguousarray(wave, dtype=np.float32)
    nf = num_frames(wave.size, frame_length, frame_shift)
    idx = np.arange(frame_length)[None, :] + frame_shift * np.arange(nf)[:, None]
    return wave[idx]                                                     # (nf, frame_length) float32


def fbank_f64(wave, num_bins=40, sample_rate=16000, frame_length=400, frame_shift=160, window=0, log=True):
    """The same pipeline evaluated in float64 (tables as the reference builds them: its float32 mel weights -- mel_bank --, the window rounded to
    float32; per-frame arithmetic and the FFT in double): what both the reference's float32 recurrence-twiddle FFT and the HIP
    kernel's exactly-rounded one approximate.  The arbiter of the GPU tests (tests/test_hip_fbank_f64.py, the fuzz test of
    tests/test_hip_fbank.py): every bin of the kernel is held to it in the unit of fbank_units.  log=False: the mel energies
    before the floor and the logarithm."""
    n, W, win = _tables(num_bins, sample_rate, frame_length, window)
    x = _frames(wave, frame_length, frame_shift).astype(np.float64)
    if not x.shape[0]:
        return np.empty((0, num_bins), np.float64)
    x = x - x.mean(axis=1, keepdims=True)
    c = np.float64(np.float32(0.97))                                     # fbank.h:122-127 (the constant is 0.97f)
    x = np.concatenate([x[:, :1] - c * x[:, :1], x[:, 1:] - c * x[:, :-1]], axis=1)
    spec = np.fft.fft(np.concatenate([x * win.astype(np.float64), np.zeros((x.shape[0], n - frame_length))], axis=1), axis=1)[:, :n // 2]
    e = (spec.real ** 2 + spec.imag ** 2) @ W.astype(np.float64).T
    return np.log(np.maximum(e, np.finfo(np.float32).eps)) if log else e


EPS32 = float(np.finfo(np.float32).eps)


def fbank_noise_scale(wave, num_bins=40, sample_rate=16000, frame_length=400, frame_shift=160, window=0):
    """S per (frame, bin): what float32 rounding of the DC-removed, windowed frame leaves in a mel bin as white noise,
    S = (sum_k W[b, k]) eps^2 sum_i ((x_i - mean) win_i)^2 -- each of the frame's samples carries a rounding error of relative
    size eps = 2^-23, the transform spreads their energy evenly over its bins, a mel bin collects sum_k W[b, k] of them."""
    _, W, win = _tables(num_bins, sample_rate, frame_length, window)
    x = _frames(wave, frame_length, frame_shift).astype(np.float64)
    x = (x - x.mean(axis=1, keepdims=True)) * win.astype(np.float64) if x.shape[0] else x
    return EPS32 ** 2 * (x ** 2).sum(axis=1)[:, None] * W.astype(np.float64).sum(axis=1)[None, :]


def fbank_units(got, wave, num_bins=40, sample_rate=16000, frame_length=400, frame_shift=160, window=0):
    """Error of log-mel features `got` (frames, bins) against the float64 evaluation, per bin, in units of the noise a correct
    float32 pipeline cannot avoid:  u = |exp(got) - E| / (2 sqrt(E S) + S + eps E)  with E = max(float64 mel energy, FLT_EPSILON)
    and S = fbank_noise_scale: eps E is one rounding of a loud bin, S and the cross term 2 sqrt(E S) what the frame's rounding
    noise adds to a bin far below the frame's peak.  Silence compares at the floor through the same formula.  Non-finite -> inf."""
    cfg = (num_bins, sample_rate, frame_length, frame_shift, window)
    E = np.maximum(fbank_f64(wave, *cfg, log=False), EPS32)
    S = fbank_noise_scale(wave, *cfg)
    got = np.asarray(got, np.float64)
    assert got.shape == E.shape, (got.shape, E.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        u = np.abs(np.exp(got) - E) / (2.0 * np.sqrt(E * S) + S + EPS32 * E)
    return np.where(np.isfinite(u), u, np.inf)


def recurrence_twiddles(n, count=None):
    """e^{-2 pi i j / n}, j = 0 .. count - 1 (default n / 2; at most n), as (cos, -sin) float32 pairs from a float32 quarter-wave recurrence -- the way the
    reference builds the sine table of its FFT (restated in fbank_oracle.c::sine_table) -- instead of rounding each value from
    double.  The negative control of the tight bar: the kernel's two twiddle tables rebuilt like this must miss it."""
    f32 = np.float32
    n4, n8 = n // 4, n // 8
    tbl = np.zeros(n + n4, np.float32)
    t = f32(np.sin(np.pi / n))
    dc = f32(2) * t * t
    ds = f32(np.sqrt(dc * (f32(2) - dc)))
    t = f32(2) * dc
    c, s = f32(1), f32(0)
    tbl[n4] = 1
    for i in range(1, n8):
        c = f32(c - dc); dc = f32(dc + t * c)
        s = f32(s + ds); ds = f32(ds - t * s)
        tbl[i], tbl[n4 - i] = s, c
    tbl[n8] = f32(np.sqrt(0.5))
    for i in range(n4):
        tbl[n // 2 - i] = tbl[i]
    tbl[n // 2:n] = -tbl[:n // 2]
    tbl[n:] = tbl[:n4]
    j = np.arange(n // 2 if count is None else count)
    return np.stack([tbl[j + n4], -tbl[j]], axis=1).astype(np.float32)


def exact_twiddles(n, count=None):
    j = np.arange(n // 2 if count is None else count, dtype=np.float64)
    return np.stack([np.cos(2 * np.pi * j / n), -np.sin(2 * np.pi * j / n)], axis=1).astype(np.float32)


def coarse_twiddles(n, count=None):
    """The exact values rounded to multiples of 2^-18 (32 float32 ulps of 1: a twiddle table of too few bits)."""
    j = np.arange(n // 2 if count is None else count, dtype=np.float64)
    t = np.stack([np.cos(2 * np.pi * j / n), -np.sin(2 * np.pi * j / n)], axis=1)
    return (np.round(t * 2.0 ** 18) / 2.0 ** 18).astype(np.float32)


TWIDDLES = dict(exact=exact_twiddles, recurrence=recurrence_twiddles, coarse=coarse_twiddles)


def _table_rfft512(x, tw256, tw512):
    """512-point real transform of float32 rows the way the kernel factors it -- the frame packed as 256 complex values, a
    256-point complex transform (here plain radix-2 decimation in frequency), the untangle pass with the 512-point twiddles --
    every operation in float32 with the twiddles taken from the given tables: the CPU emulation of the twiddle control."""
    z = (x[:, 0::2] + 1j * x[:, 1::2]).astype(np.complex64)              # (rows, 256)
    w = (tw256[:, 0] + 1j * tw256[:, 1]).astype(np.complex64)            # e^{-2 pi i j / 256}, j < 128
    rows, half = z.shape[0], 128
    z = z.reshape(rows, 1, 256)
    while half >= 1:                                                     # blocks of 2 half: (a, b) -> (a + b, (a - b) w^(j 128 / half))
        a, b = z[:, :, :half], z[:, :, half:]
        tw = w[::128 // half][None, None, :half]
        z = np.concatenate([(a + b).astype(np.complex64), ((a - b).astype(np.complex64) * tw).astype(np.complex64)], axis=2)
        z = z.reshape(rows, -1, half) if half > 1 else z.reshape(rows, -1)
        half //= 2
    rev = np.array([int(format(k, "08b")[::-1], 2) for k in range(256)])
    Z = z[:, rev]                                                        # natural order
    Zn = np.conj(Z[:, (256 - np.arange(256)) % 256])
    u = (tw512[:, 0] + 1j * tw512[:, 1]).astype(np.complex64)            # e^{-2 pi i k / 512}, k < 256
    e, o = (Z + Zn).astype(np.complex64), (Z - Zn).astype(np.complex64)
    return (np.complex64(0.5) * e + (np.complex64(-0.5j) * u)[None, :] * o).astype(np.complex64)


def fbank_f32_exact(wave, num_bins=40, sample_rate=16000, frame_length=400, frame_shift=160, window=0, fft="pocketfft",
                    twiddles="exact", mel="float32", weight=None):
    """A plain float32 restatement with exactly rounded twiddles: pocketfft on complex64, everything else in np.float32.  It
    calibrates the tight bar from the reference side (what does a correct float32 pipeline reach in fbank_units?) and hosts the
    CPU emulation of the negative controls:
      fft="table", twiddles="recurrence"   the transform factored like the kernel's, its twiddles from recurrence_twiddles
      fft="table", twiddles="coarse"       ... from coarse_twiddles
      mel="double"                         the mel bank computed in double, then rounded
      weight=(bin, factor)                 the centre weight of one filter times `factor`"""
    f32 = np.float32
    n, W, win = _tables(num_bins, sample_rate, frame_length, window, mel == "double")
    if weight is not None:
        b, factor = weight
        W = W.copy()
        W[b, int(np.argmax(W[b]))] *= f32(factor)
    x = _frames(wave, frame_length, frame_shift)
    if not x.shape[0]:
        return np.empty((0, num_bins), np.float32)
    x = x - (x.sum(axis=1, dtype=f32, keepdims=True) / f32(frame_length))
    x = np.concatenate([x[:, :1] - f32(0.97) * x[:, :1], x[:, 1:] - f32(0.97) * x[:, :-1]], axis=1).astype(f32)
    x = np.concatenate([x * win, np.zeros((x.shape[0], n - frame_length), f32)], axis=1).astype(f32)
    if fft == "pocketfft":
        import scipy.fft                                                 # (numpy's own fft computes in double; scipy's keeps complex64)
        spec = scipy.fft.fft(x.astype(np.complex64), axis=1)[:, :n // 2]
        assert spec.dtype == np.complex64
    else:
        make = TWIDDLES[twiddles]
        full = np.concatenate([x, np.zeros((x.shape[0], 512 - n), f32)], axis=1)
        spec = _table_rfft512(full, make(256), make(512))[:, ::512 // n]
    power = (spec.real * spec.real + spec.imag * spec.imag).astype(f32)
    e = (power @ W.T).astype(f32)
    return np.log(np.maximum(e, f32(EPS32))).astype(f32)
