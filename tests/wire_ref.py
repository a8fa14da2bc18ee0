"""An independent numpy restatement of the wire encodings (include/wekws_hip.h: enum wekws_hip_wire): how the bytes a stream
arrives in become int16 samples.  Vectorised integer arithmetic written from the table, sharing no code with the library; the
tests hold wekws_hip_wire_decode and the rate bank's fetch to it."""
import numpy as np

ENCODINGS = ("s16", "mulaw", "alaw", "u8", "f32")
BYTES = {"s16": 2, "mulaw": 1, "alaw": 1, "u8": 1, "f32": 4}
DTYPE = {"s16": np.dtype("<i2"), "mulaw": np.dtype(np.uint8), "alaw": np.dtype(np.uint8), "u8": np.dtype(np.uint8),
         "f32": np.dtype("<f4")}


def mulaw(c):
    u = (~np.asarray(c, dtype=np.int64)) & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84)


def alaw(c):
    a = np.asarray(c, dtype=np.int64) ^ 0x55
    t = (a & 0x0F) << 4
    s = (a & 0x70) >> 4
    t = t + np.where(s > 0, 0x108, 8)
    t = np.where(s > 1, t << np.maximum(s - 1, 0), t)
    return np.where(a & 0x80, t, -t)


def u8(c):
    return (np.asarray(c, dtype=np.int64) - 128) * 256


def f32(x):
    """rint(x * 32768) half to even, saturated, NaN -> 0.  The product of a float32 with 2^15 is exact in float64 too, and
    np.rint rounds half to even: no float32 arithmetic is needed to restate it."""
    with np.errstate(invalid="ignore", over="ignore"):             # (signalling NaNs among the inputs)
        x = np.asarray(x, dtype=np.float32).astype(np.float64)
        r = np.rint(x * 32768.0)
    r = np.where(np.isnan(r), 0.0, np.clip(r, -32768.0, 32767.0))
    return r.astype(np.int64)


def decode(encoding, raw):
    """``raw``: bytes, or a numpy array of the encoding's own dtype -> int16 samples (len(raw) // bytes of them)."""
    if encoding not in ENCODINGS:
        raise ValueError(encoding)
    dt = DTYPE[encoding]
    if isinstance(raw, (bytes, bytearray, memoryview)):
        raw = bytes(raw)
        raw = np.frombuffer(raw[:len(raw) // dt.itemsize * dt.itemsize], dtype=dt)
    a = np.asarray(raw)
    assert a.dtype == dt, (a.dtype, dt)
    v = {"s16": lambda z: z.astype(np.int64), "mulaw": mulaw, "alaw": alaw, "u8": u8, "f32": f32}[encoding](a)
    assert v.min(initial=0) >= -32768 and v.max(initial=0) <= 32767
    return v.astype(np.int16)


def encode_bytes(encoding, values):
    """Host values as the bytes of a wire row (test inputs): uint8 codes, int16 samples or float32 values."""
    return np.ascontiguousarray(np.asarray(values).astype(DTYPE[encoding])).view(np.uint8)


# float32 inputs whose value the table pins: (x, v)
F32_CASES = [
    (1.0, 32767), (-1.0, -32768), (1.5 / 32768, 2), (2.5 / 32768, 2), (-0.5 / 32768, 0), (0.5 / 32768, 0), (-1.5 / 32768, -2),
    (32767.5 / 32768, 32767), (32766.5 / 32768, 32766), (float("nan"), 0), (float("inf"), 32767), (float("-inf"), -32768),
    (1e-45, 0), (-1e-45, 0), (1.1754942e-38, 0), (3.0e38, 32767), (-3.0e38, -32768), (0.0, 0), (-0.0, 0), (0.25, 8192),
    (-0.999969482421875, -32767),
]
