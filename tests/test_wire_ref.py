"""CPU: the numpy restatement of the wire encodings (tests/wire_ref.py) against the anchors of the definition, against Python's
own G.711 tables where the interpreter still ships them, and on the float32 values the definition pins."""
import numpy as np
import pytest

from tests import wire_ref as WR

CODES = np.arange(256, dtype=np.uint8)


def test_anchor_values():
    mu = WR.decode("mulaw", CODES)
    assert (mu[0xFF], mu[0x7F], mu[0x80], mu[0x00]) == (0, 0, 32124, -32124)
    al = WR.decode("alaw", CODES)
    assert (al[0xD5], al[0x55], al[0xAA], al[0x2A]) == (8, -8, 32256, -32256)
    u = WR.decode("u8", CODES)
    assert (u[0], u[128], u[255], u[127]) == (-32768, 0, 32512, -256)
    assert mu.dtype == al.dtype == u.dtype == np.int16
    # G.711 is odd-symmetric in its sign bit and monotone within a sign
    assert np.array_equal(mu[:128], -mu[128:]) and (np.diff(mu[128:].astype(int)) < 0).all()
    assert np.array_equal(al[:128][::1], -al[128:]) and len(set(al.tolist())) == 256 and len(set(mu.tolist())) == 255


def test_g711_tables_equal_audioop():
    audioop = pytest.importorskip("audioop")
    raw = CODES.tobytes()
    assert np.array_equal(WR.decode("mulaw", raw), np.frombuffer(audioop.ulaw2lin(raw, 2), dtype=np.int16))
    assert np.array_equal(WR.decode("alaw", raw), np.frombuffer(audioop.alaw2lin(raw, 2), dtype=np.int16))


def test_s16_is_little_endian_and_odd_bytes_are_dropped():
    assert WR.decode("s16", bytes([0x34, 0x12, 0x00, 0x80, 0xFF])).tolist() == [0x1234, -32768]
    assert WR.decode("f32", np.float32(0.5).tobytes() + b"\x00").tolist() == [16384]
    assert WR.decode("mulaw", b"").size == 0


def test_f32_cases():
    x = np.asarray([c[0] for c in WR.F32_CASES], dtype=np.float32)
    want = [c[1] for c in WR.F32_CASES]
    assert WR.decode("f32", x).tolist() == want
    assert WR.decode("f32", x.tobytes()).tolist() == want
    # the named ones, spelled out: the ends, ties to even, saturation, NaN, Inf, denormals
    one = lambda v: int(WR.decode("f32", np.asarray([v], dtype=np.float32))[0])
    assert (one(1.0), one(-1.0)) == (32767, -32768)
    assert (one(1.5 / 32768), one(2.5 / 32768), one(-0.5 / 32768)) == (2, 2, 0)
    assert one(32767.5 / 32768) == 32767
    assert one(np.nan) == 0 and (one(np.inf), one(-np.inf)) == (32767, -32768)
    assert one(np.float32(1e-45)) == 0 and one(np.finfo(np.float32).tiny / 2) == 0
    # every int16 value survives the round trip through unit-scale float
    v = np.arange(-32768, 32768)
    assert np.array_equal(WR.decode("f32", (v / 32768.0).astype(np.float32)), v.astype(np.int16))
