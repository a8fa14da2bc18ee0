"""CPU: the resampler's definition and its host plan (wekws_amd/csrc/resample_plan.h), without a device.

The float64 restatement of torchaudio's Resample (tests/resample_ref.py) is held to scipy.signal.upfirdn and to an ideal
tone; the library's taps, live ranges, output counts and streaming plan -- reached through the debug entry points of the
hooks library -- are held to the restatement."""
import ctypes as C
import math
import os

import numpy as np
import pytest
from scipy import signal

from tests import resample_ref as RR
from wekws_amd import _capi

HOOKS = os.path.join(os.path.dirname(_capi.lib_path()), "libwekws_hip_hooks.so")
ALL_PAIRS = [(r, 16000) for r in (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000)] + [(16000, 8000), (16000, 16000)]


@pytest.fixture(scope="module")
def hooks():
    lib = C.CDLL(HOOKS)
    lib.wekws_hip_debug_resample_plan.restype = C.c_int
    lib.wekws_hip_debug_resample_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int64,
                                                  C.c_void_p, C.c_void_p, C.c_int64]
    lib.wekws_hip_debug_resample_step.restype = C.c_int
    lib.wekws_hip_debug_resample_step.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    lib.wekws_hip_debug_resample_schedule.restype = C.c_int
    lib.wekws_hip_debug_resample_schedule.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                      C.c_void_p]
    return lib


def lib_plan(hooks, orig, new, taps=True):
    dims = np.zeros(10, dtype=np.int64)
    assert hooks.wekws_hip_debug_resample_plan(orig, new, 6, 0.99, dims.ctypes.data, None, 0, None, None, 0) == 0
    o, n, width, K = (int(v) for v in dims[:4])
    k = np.zeros((n, K), dtype=np.float32)
    first, last = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    assert hooks.wekws_hip_debug_resample_plan(orig, new, 6, 0.99, dims.ctypes.data, k.ctypes.data if taps else None, k.size,
                                               first.ctypes.data, last.ctypes.data, n) == 0
    return dims, k, first, last


# ------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("orig,new", RR.PAIRS)
def test_restatement_is_upfirdn_with_the_same_taps(orig, new):
    """y = downsample_o(h * upsample_n(x)) with the taps laid out on the common grid: h[(m - width) n - i o + c] = k[i][m]."""
    p = RR.Plan(orig, new)
    rng = np.random.default_rng(orig)
    x = rng.uniform(-1e4, 1e4, size=3001)
    k = p.taps.astype(np.float64)
    c = (p.n - 1) * p.o + p.width * p.n                      # grid index of the earliest tap (i = n - 1, m = 0), negated
    h = np.zeros(c + (p.K - 1 - p.width) * p.n + 1)
    for i in range(p.n):
        for m in range(p.K):
            pos = (m - p.width) * p.n - i * p.o
            # y[j n + i] = sum_m k[i][m] x[j o + m - width]: on the grid of rate n orig, x[s] sits at s n, output q at q o;
            # tap m of phase i is at offset (j o + m - width) n - (j n + i) o = pos from the output
            if h[pos + c] != 0.0:
                assert h[pos + c] == k[i, m]                 # two (i, m) on one grid point carry the same tap
            h[pos + c] = k[i, m]
    # upfirdn computes y_full[t] = sum_s h[t - s n] x[s] on the grid; output q (grid q o) wants sum_s h[s n - q o + c] x[s]:
    # h is symmetric in construction only up to rounding, so flip it and read at t = q o + (len(h) - 1 - c)
    full = signal.upfirdn(h[::-1], x, up=p.n, down=1)
    off = h.size - 1 - c
    want, _ = RR.resample(p, x)
    idx = np.arange(want.size) * p.o + off
    got = np.where(idx < full.size, full[np.minimum(idx, full.size - 1)], 0.0)
    err = float(np.abs(got - want).max()) / float(np.abs(x).max())
    print(f"{orig}->{new}: restatement vs upfirdn {err:.3e} of the peak")
    assert want.size == p.num_samples(x.size) and err <= 1e-9


@pytest.mark.parametrize("orig,new", RR.PAIRS)
def test_a_tone_comes_out_as_the_tone(orig, new):
    p = RR.Plan(orig, new)
    L = orig // 4
    x = 1000.0 * np.sin(2 * np.pi * 440.0 * np.arange(L) / orig)
    y, _ = RR.resample(p, x)
    ideal = 1000.0 * np.sin(2 * np.pi * 440.0 * np.arange(y.size) / new)
    edge = int(math.ceil(2 * p.lpw * new / min(orig, new))) + 2
    err = float(np.abs(y - ideal)[edge:-edge].max()) / 1000.0
    print(f"{orig}->{new}: 440 Hz tone {err:.3e} of the amplitude")
    assert err <= 1e-3


# ------------------------------------------------------------------------------------------ the library's plan
@pytest.mark.parametrize("orig,new", ALL_PAIRS)
def test_taps_and_live_ranges(hooks, orig, new):
    p = RR.Plan(orig, new)
    dims, k, first, last = lib_plan(hooks, orig, new)
    assert tuple(int(v) for v in dims[:4]) == (p.o, p.n, p.width, p.K)
    assert np.array_equal(first, p.first) and np.array_equal(last, p.last)
    assert int(dims[4]) == int((p.last - p.first + 1).max()) and int(dims[5]) % 2 == 1 and int(dims[5]) >= int(dims[4])
    assert (k[~p.live] == 0).all(), "a tap under the active clamp is exactly 0"
    ulp = np.spacing(np.abs(p.taps))
    assert (np.abs(k.astype(np.float64) - p.taps.astype(np.float64)) <= ulp)[p.live].all()
    assert int(dims[6]) <= 64 * 1024                        # every supported pair fits the LDS budget
    if (orig, new) == (44100, 16000):
        assert sorted(set((p.last - p.first + 1).tolist())) == [33, 34] and p.K == 475
    if (orig, new) == (48000, 16000):
        assert (p.last - p.first + 1).tolist() == [37] and p.K == 41


def test_num_samples_is_exact_in_64_bits():
    lib = _capi.load()
    rng = np.random.default_rng(0)
    for orig, new in ALL_PAIRS + [(44101, 16000), (16000, 44100)]:
        p = RR.Plan(orig, new) if (orig, new) in ALL_PAIRS else None
        g = math.gcd(orig, new)
        for L in [0, 1, 2, orig // g - 1, orig // g, orig // g + 1, 2 ** 31 - 1, 2 ** 40 + 7] + [int(v) for v in rng.integers(0, 2 ** 33, 50)]:
            want = -((-new * L) // orig)
            assert lib.wekws_hip_resample_num_samples(orig, new, L) == want, (orig, new, L)
            if p is not None:
                assert p.num_samples(L) == want
    L = 2 ** 31 - 1                                         # 160 L overflows int32 (and 16000 L int64's neighbourhood is far)
    assert lib.wekws_hip_resample_num_samples(44100, 16000, L) == (160 * L + 440) // 441 == 779132389
    assert lib.wekws_hip_resample_num_samples(0, 16000, 5) == -1 and lib.wekws_hip_resample_num_samples(16000, 8000, -1) == -1


def schedules(rng, p, count, max_chunk):
    """chunk sizes 0, 1, below the width, prime, and up to max_chunk"""
    primes = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 211, 307, 401, 503]
    for _ in range(count):
        kind = rng.integers(0, 5)
        n = int(rng.integers(1, 14))
        if kind == 0:
            ch = rng.integers(0, 2, n)
        elif kind == 1:
            ch = rng.integers(0, max(p.width, 2), n)
        elif kind == 2:
            ch = rng.choice(primes, n)
        elif kind == 3:
            ch = rng.integers(0, max_chunk + 1, n)
        else:
            ch = rng.choice([0, 1, max_chunk, max_chunk - 1, p.width, p.o, p.K], n)
        yield np.ascontiguousarray(ch, dtype=np.int32)


@pytest.mark.parametrize("orig,new", RR.PAIRS + ((16000, 16000),))
def test_streaming_plan_over_seeded_schedules(hooks, orig, new):
    p = RR.Plan(orig, new)
    dims, _, _, _ = lib_plan(hooks, orig, new, taps=False)
    hist_cap, max_live = int(dims[8]), int(dims[4])
    rng = np.random.default_rng(orig + new)
    worst_look, worst_hist = 0, 0
    for ch in schedules(rng, p, 400, 1200):                  # 5 pairs x 400 = 2,000 schedules
        totals, keeps = np.zeros(ch.size, dtype=np.int64), np.zeros(ch.size, dtype=np.int64)
        assert hooks.wekws_hip_debug_resample_schedule(orig, new, 6, 0.99, ch.ctypes.data, ch.size, 1, totals.ctypes.data,
                                                       keeps.ctypes.data) == 0
        N, emitted, keep = 0, 0, 0
        for k, c in enumerate(ch.tolist()):
            flush = k == ch.size - 1
            want_total, want_keep = p.step(N, c, flush)
            N += c
            assert (int(totals[k]), int(keeps[k])) == (want_total, want_keep), (ch.tolist(), k)
            assert want_total >= emitted and want_keep >= keep and want_total <= p.num_samples(N)
            out = np.zeros(4, dtype=np.int64)
            assert hooks.wekws_hip_debug_resample_step(orig, new, 6, 0.99, N - c, c, int(flush), out.ctypes.data) == 0
            assert want_total - emitted <= int(out[3]), "max_out always suffices"
            emitted, keep = want_total, want_keep
            if not flush:
                # every output not yet emitted finds its live taps in what the stream keeps; what it keeps fits
                assert keep <= max(p.lo(emitted), 0) and N - keep < max_live <= hist_cap
                # the look-ahead: received samples at or past the next output's position (the kept history, the line above, is
                # bounded by the live taps of a phase, about twice as many)
                look = N - math.ceil(emitted * p.o / p.n)
                assert look <= p.lookahead_bound(), ("look-ahead", ch.tolist(), k, look)
                worst_look, worst_hist = max(worst_look, look), max(worst_hist, N - keep)
        assert emitted == p.num_samples(N)                      # counts sum to the one-shot count after the flush
    print(f"{orig}->{new}: look-ahead {worst_look} <= {p.lookahead_bound()}, history kept {worst_hist} < {max_live}")


def test_need_is_non_decreasing():
    """the closed form (a bisection in the library) rests on it"""
    for orig, new in ALL_PAIRS:
        p = RR.Plan(orig, new)
        need = [p.need(q) for q in range(3 * p.n + 1)]
        lo = [p.lo(q) for q in range(3 * p.n + 1)]
        assert all(b >= a for a, b in zip(need, need[1:])) and all(b >= a for a, b in zip(lo, lo[1:]))


# ------------------------------------------------------------------------------------------ creation
def make_cfg(orig, new, max_streams=0, max_chunk=0, lpw=6, rolloff=0.99, out=0):
    c = _capi.ResampleCfg()
    c.orig_freq, c.new_freq, c.lowpass_filter_width, c.out_dtype, c.rolloff = orig, new, lpw, out, rolloff
    c.max_streams, c.max_chunk, c.device = max_streams, max_chunk, 0
    return c


def test_create_time_refusals():
    import torch
    lib = _capi.load()
    assert C.sizeof(_capi.ResampleCfg) == 48
    h = C.c_void_p()
    for orig, new in ((0, 16000), (-8000, 16000), (16000, 0), (16000, -1)):
        assert lib.wekws_hip_resample_create(C.byref(make_cfg(orig, new)), C.byref(h)) == -1 and not h
        assert "rates are positive" in _capi.last_error()
    assert lib.wekws_hip_resample_create(C.byref(make_cfg(44101, 16000)), C.byref(h)) == -4 and not h     # EUNSUPPORTED
    assert "LDS" in _capi.last_error() and "16000 phases" in _capi.last_error()
    for mc in (0, -5):
        assert lib.wekws_hip_resample_create(C.byref(make_cfg(48000, 16000, max_streams=4, max_chunk=mc)), C.byref(h)) == -1
        assert "max_chunk" in _capi.last_error()
    assert lib.wekws_hip_resample_create(C.byref(make_cfg(48000, 16000, lpw=0)), C.byref(h)) == -1
    assert lib.wekws_hip_resample_create(C.byref(make_cfg(48000, 16000, out=7)), C.byref(h)) == -1
    assert lib.wekws_hip_resample_create(None, C.byref(h)) == -1
    if not torch.cuda.is_available():
        # a supported pair gets as far as the device
        for orig, new in ALL_PAIRS:
            assert lib.wekws_hip_resample_create(C.byref(make_cfg(orig, new, 8, 4800)), C.byref(h)) == -3 and not h, (orig, new)
    assert lib.wekws_hip_resample_push(None, None, 1, 1, None, None, 0, None, 0, None, None) == -1
    assert lib.wekws_hip_resample_compute(None, None, 1, 1, None, None, 0, None) == -1
    assert lib.wekws_hip_resample_max_out(None, 5, 0) == 0


def test_symbols_and_signatures():
    lib = _capi.load()
    names = ["create", "destroy", "num_samples", "compute", "compute_i16", "push", "max_out", "reset", "counts"]
    for n in names:
        assert hasattr(lib, "wekws_hip_resample_" + n) and "wekws_hip_resample_" + n in _capi.SIGNATURES
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wekws_hip.h")).read()
    assert "#define WEKWS_HIP_ABI_VERSION 2" in src
    # the debug entry points are the hooks library's alone
    assert not hasattr(lib, "wekws_hip_debug_resample_plan") and "wekws_hip_debug" not in src
