"""CPU: the wire encodings on the host side of the C ABI, without a device -- the exported symbols, wekws_hip_wire_decode against
the numpy restatement (tests/wire_ref.py), the creation-time refusals of wekws_hip_resample_bank_create_wire, and the
call-time refusals of the _wire calls through the function every call checks its rows with (the hooks library's
wekws_hip_debug_resample_bank_check_rows)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import wire_ref as WR
from wekws_amd import _capi
from wekws_amd import frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = os.path.join(os.path.dirname(_capi.lib_path()), "libwekws_hip_hooks.so")
NAMES = ["wire_sample_bytes", "wire_decode", "resample_bank_create_wire", "resample_bank_compute_wire", "resample_bank_push_wire",
         "resample_bank_encoding_of"]
ENC = {n: i for i, n in enumerate(WR.ENCODINGS)}
OK, ALIGN, WIDTH, MEMBER, LENGTH, ENCODING = range(6)


@pytest.fixture(scope="module")
def hooks():
    lib = C.CDLL(HOOKS)
    lib.wekws_hip_debug_resample_bank_check_rows.restype = C.c_int
    lib.wekws_hip_debug_resample_bank_check_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                                             C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64,
                                                             C.c_void_p]
    return lib


def check_rows(hooks, bank, wire_call, addr, width, nsamp, members, limit=2 ** 30 - 1):
    rates = np.asarray([r for r, _ in bank], dtype=np.int32)
    encs = np.asarray([ENC[e] for _, e in bank], dtype=np.int32)
    mem = np.ascontiguousarray(members, dtype=np.int32)
    ns = None if nsamp is None else np.ascontiguousarray(nsamp, dtype=np.int32)
    out = np.full(4, -9, dtype=np.int64)
    rc = hooks.wekws_hip_debug_resample_bank_check_rows(rates.ctypes.data, encs.ctypes.data, rates.size, 16000, 6, 0.99, int(wire_call),
                                                        addr, width, None if ns is None else ns.ctypes.data, mem.ctypes.data, mem.size,
                                                        limit, out.ctypes.data)
    return rc, int(out[0]), int(out[1])


def make_cfg(orig, max_streams=0, max_chunk=0):
    c = _capi.ResampleCfg()
    c.orig_freq, c.new_freq, c.lowpass_filter_width, c.rolloff, c.out_dtype = orig, 16000, 6, 0.99, 0
    c.max_streams, c.max_chunk, c.device = max_streams, max_chunk, 0
    return c


def create_wire(lib, bank, cfg=None):
    rates = (C.c_int32 * max(len(bank), 1))(*[r for r, _ in bank])
    encs = (C.c_int32 * max(len(bank), 1))(*[e if isinstance(e, int) else ENC[e] for _, e in bank])
    h = C.c_void_p(0x1234)
    rc = lib.wekws_hip_resample_bank_create_wire(C.byref(cfg or make_cfg(bank[0][0] if bank else 48000)), rates, encs, len(bank), C.byref(h))
    return rc, h


def test_symbols_are_exported_and_bound():
    lib = _capi.load()
    src = open(os.path.join(ROOT, "include", "wekws_hip.h")).read()
    for n in NAMES:
        name = "wekws_hip_" + n
        assert hasattr(lib, name) and name in _capi.SIGNATURES and name + "(" in src, name
    assert "#define WEKWS_HIP_ABI_VERSION 2" in src
    for i, n in enumerate(("S16", "MULAW", "ALAW", "U8", "F32")):
        assert f"WEKWS_HIP_WIRE_{n} = {i}" in src
    assert frontend.ENCODINGS == WR.ENCODINGS == ("s16", "mulaw", "alaw", "u8", "f32")
    hooks = C.CDLL(HOOKS)
    assert hasattr(hooks, "wekws_hip_debug_resample_bank_check_rows") and not hasattr(lib, "wekws_hip_debug_resample_bank_check_rows")
    assert "wekws_hip_debug" not in src


def test_sample_bytes():
    lib = _capi.load()
    assert [lib.wekws_hip_wire_sample_bytes(i) for i in range(5)] == [2, 1, 1, 1, 4] == [WR.BYTES[e] for e in WR.ENCODINGS]
    assert [lib.wekws_hip_wire_sample_bytes(i) for i in (-1, 5, 6, 255, 2 ** 31 - 1)] == [0] * 5


def lib_decode(enc, raw):
    lib = _capi.load()
    raw = np.ascontiguousarray(np.frombuffer(bytes(raw), dtype=np.uint8))
    n = raw.size // WR.BYTES[enc]
    out = np.full(n + 1, -77, dtype=np.int16)
    assert lib.wekws_hip_wire_decode(ENC[enc], raw.ctypes.data if raw.size else None, n, out.ctypes.data) == 0
    assert out[n] == -77, "nothing is written past n samples"
    return out[:n]


def test_decode_equals_the_restatement():
    codes = np.arange(256, dtype=np.uint8).tobytes()
    for enc in ("mulaw", "alaw", "u8"):
        assert np.array_equal(lib_decode(enc, codes), WR.decode(enc, codes)), enc
    x = np.asarray([c[0] for c in WR.F32_CASES], dtype=np.float32)
    assert lib_decode("f32", x.tobytes()).tolist() == [c[1] for c in WR.F32_CASES] == WR.decode("f32", x).tolist()
    rng = np.random.default_rng(7)
    wild = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32)      # every exponent, NaNs among them
    near = ((rng.integers(-2 * 32768, 2 * 32768, 20000) + rng.choice([0.0, 0.5, 0.25, -0.5], 20000)) / 32768.0).astype(np.float32)
    for v in (wild, near):
        assert np.array_equal(lib_decode("f32", v.tobytes()), WR.decode("f32", v))
    s = rng.integers(-32768, 32768, 1000).astype("<i2")
    assert np.array_equal(lib_decode("s16", s.tobytes()), s)
    # an unaligned source is read byte by byte
    assert np.array_equal(lib_decode("s16", (b"\x00" + s.tobytes())[1:]), s)
    assert lib_decode("mulaw", b"").size == 0
    lib = _capi.load()
    out = np.zeros(4, dtype=np.int16)
    assert lib.wekws_hip_wire_decode(5, codes, 4, out.ctypes.data) == -1 and "encoding" in _capi.last_error()
    assert lib.wekws_hip_wire_decode(1, codes, -1, out.ctypes.data) == -1
    assert lib.wekws_hip_wire_decode(1, None, 4, out.ctypes.data) == -1 and lib.wekws_hip_wire_decode(1, codes, 4, None) == -1


def test_create_time_refusals():
    import torch
    lib = _capi.load()
    for bank, what in (([(8000, 5)], "encoding"), ([(8000, "mulaw"), (16000, -1)], "member 1"),
                       ([(8000, "mulaw"), (16000, "s16"), (8000, "mulaw")], "repeats the pair (8000, mulaw)"),
                       ([], "1..16"), ([(8000 + k, "u8") for k in range(17)], "1..16"), ([(0, "alaw")], "positive")):
        rc, h = create_wire(lib, bank)
        assert rc == -1 and not h and what in _capi.last_error(), (bank, rc, _capi.last_error())
    rc, h = create_wire(lib, [(48000, "f32"), (44101, "mulaw")])
    assert rc == -4 and not h and "member 1" in _capi.last_error() and "44101" in _capi.last_error()
    h = C.c_void_p(0x1234)
    rates = (C.c_int32 * 1)(8000)
    assert lib.wekws_hip_resample_bank_create_wire(C.byref(make_cfg(8000)), rates, None, 1, C.byref(h)) == -1 and not h
    # the int16 entry point keeps its own words for a repeated rate
    assert lib.wekws_hip_resample_bank_create(C.byref(make_cfg(8000)), (C.c_int32 * 2)(8000, 8000), 2, C.byref(h)) == -1
    assert "repeats the rate 8000" in _capi.last_error()
    if not torch.cuda.is_available():
        # the same rate under two encodings is a bank: it gets as far as the device
        for bank, ms in (([(8000, "mulaw"), (8000, "alaw"), (8000, "s16"), (8000, "u8"), (8000, "f32")], 4),
                         ([(8000, "mulaw"), (16000, "s16"), (48000, "f32")], 0)):
            rc, h = create_wire(lib, bank, make_cfg(bank[0][0], max_streams=ms, max_chunk=160 if ms else 0))
            assert rc == -3 and not h, (bank, rc, _capi.last_error())
    assert lib.wekws_hip_resample_bank_push_wire(None, None, 1, 4, None, None, 0, None, 0, None, None) == -1
    assert lib.wekws_hip_resample_bank_compute_wire(None, None, 1, 4, None, None, None, 0, None) == -1
    assert lib.wekws_hip_resample_bank_encoding_of(None, 0) == -1


BANK = [(8000, "mulaw"), (8000, "s16"), (48000, "f32"), (8000, "u8")]


def test_call_time_refusals(hooks):
    A = 0x7F0000001000                                              # a device address, 4096-aligned
    # an accepted call: every row exactly as full as its bytes allow
    assert check_rows(hooks, BANK, 1, A, 160, [160, 80, 40, 160], [0, 1, 2, 3]) == (0, OK, -1)
    assert check_rows(hooks, BANK, 1, A + 4, 160, None, [0, 1, 2, 3]) == (0, OK, -1)
    assert check_rows(hooks, BANK, 1, A, 0, [0, 0], [0, 2]) == (0, OK, -1)
    # a misaligned pointer: every phase of a dword but the first
    for off in (1, 2, 3, 5, 6, 7):
        assert check_rows(hooks, BANK, 1, A + off, 160, [1], [0]) == (0, ALIGN, -1), off
    # row_bytes % 4
    for w in (1, 2, 3, 158, 161, -4, 2 ** 30):
        assert check_rows(hooks, BANK, 1, A, w, [0], [0]) == (0, WIDTH, -1), w
    # nsamp * bytes > row_bytes, per encoding; the row is named
    assert check_rows(hooks, BANK, 1, A, 160, [160, 80, 40, 161], [0, 1, 2, 3]) == (0, LENGTH, 3)
    assert check_rows(hooks, BANK, 1, A, 160, [160, 81, 40, 160], [0, 1, 2, 3]) == (0, LENGTH, 1)
    assert check_rows(hooks, BANK, 1, A, 160, [160, 80, 41, 160], [0, 1, 2, 3]) == (0, LENGTH, 2)
    assert check_rows(hooks, BANK, 1, A, 160, [-1], [0]) == (0, LENGTH, 0)
    # ... and a push holds nsamp, in samples, against max_chunk
    assert check_rows(hooks, BANK, 1, A, 640, [160, 160], [0, 2], limit=160) == (0, OK, -1)
    assert check_rows(hooks, BANK, 1, A, 640, [160, 161], [0, 0], limit=160) == (0, LENGTH, 1)
    assert check_rows(hooks, BANK, 1, A, 160, [1, 1], [0, 4]) == (0, MEMBER, 1)
    # an int16 / float call: rows of s16 members as ever, a row of any other member refused (no alignment rule there)
    assert check_rows(hooks, BANK, 0, A + 2, 161, [161, 3], [1, 1]) == (0, OK, -1)
    assert check_rows(hooks, BANK, 0, A, 160, [160, 160], [1, 0]) == (0, ENCODING, 1)
    assert check_rows(hooks, BANK, 0, A, 160, [160], [2]) == (0, ENCODING, 0)
    assert check_rows(hooks, BANK, 0, A, 160, [161], [1]) == (0, LENGTH, 0)
    # on a bank of s16 members alone the int16 calls refuse nothing new
    assert check_rows(hooks, [(8000, "s16"), (48000, "s16")], 0, A + 2, 100, None, [0, 1, 1]) == (0, OK, -1)
    # the bank itself is planned first
    assert check_rows(hooks, [(8000, "mulaw"), (8000, "mulaw")], 1, A, 160, [1], [0])[0] == -1
    assert check_rows(hooks, [(8000, "mulaw"), (44101, "alaw")], 1, A, 160, [1], [0])[::2] == (-4, 1)
