"""GPU: wire encodings inside the rate bank's fetch (wekws_hip_resample_bank_*_wire: ResampleBank / StreamingResamplerBank fed uint8
rows of G.711, unsigned 8-bit, float32 and int16 bytes) against the int16 path fed the decoded samples, bit for bit.

The oracle of a wire row is the bank's own int16 entry point (a bank of plain rates: the path that existed before there were wire
members) on tests/wire_ref.py's decode of that row -- an independent numpy restatement of the encodings.  The bar is equality of
integer views for both output types; nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import wire_ref as WR
from tests.test_hip_resample import HOOKS
from wekws_amd import _capi
from wekws_amd.frontend import ENCODINGS, ResampleBank, StreamingResamplerBank

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEW = 16000
BANK = [(8000, "mulaw"), (8000, "alaw"), (8000, "u8"), (8000, "s16"), (48000, "f32"), (16000, "mulaw"), (44100, "s16")]
RATES = [8000, 48000, 16000, 44100]                    # the oracle's bank: the same rates, int16 alone
F32, I16 = torch.float32, torch.int16
OUT = [F32, I16]
GRIDS = [None, 1, 2]
PAD = 0xA5                                             # bytes behind a row's samples: never signal


def cap_grid(handle, grid):
    lib = C.CDLL(HOOKS)
    lib.wekws_hip_debug_resample_bank_set_grid.restype = C.c_int
    lib.wekws_hip_debug_resample_bank_set_grid.argtypes = [C.c_void_p, C.c_int]
    assert lib.wekws_hip_debug_resample_bank_set_grid(handle._ptr, grid or 0) == 0


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def raw_signal(rng, enc, n, head=None):
    """n samples of an encoding as the array a stream would carry: random codes / samples / unit-scale floats (a few of them
    beyond +-1, so that saturation is on the path), ``head`` in front."""
    if enc in ("mulaw", "alaw", "u8"):
        a = rng.integers(0, 256, n).astype(np.uint8)
    elif enc == "s16":
        a = rng.integers(-32768, 32768, n).astype("<i2")
    else:
        a = (rng.standard_normal(n) * 0.4).astype("<f4")
    if head is not None:
        head = np.asarray(head, dtype=a.dtype)[:n]
        a[:head.size] = head
    return a


def pack_rows(raws, row_bytes=None):
    """Arrays of wire samples -> one (B, row_bytes) uint8 host array, PAD behind every row's bytes."""
    rows = [np.ascontiguousarray(a).view(np.uint8) for a in raws]
    if row_bytes is None:
        row_bytes = (max([r.size for r in rows] + [0]) + 3) // 4 * 4
    host = np.full((len(rows), row_bytes), PAD, dtype=np.uint8)
    for i, r in enumerate(rows):
        host[i, :r.size] = r
    return host


def oracle_one_shot(out_dtype, raws, members):
    """Every row through the int16 entry point of a bank of plain rates, fed wire_ref's decode of the row."""
    pcm = [WR.decode(BANK[m][1], a) for a, m in zip(raws, members)]
    x = np.full((len(pcm), max([p.size for p in pcm] + [1])), 12345, dtype=np.int16)
    for i, p in enumerate(pcm):
        x[i, :p.size] = p
    ref = ResampleBank(RATES, NEW, out_dtype=out_dtype)
    y, counts = ref(torch.from_numpy(x).to(DEV), [BANK[m][0] for m in members], lengths=[p.size for p in pcm])
    torch.cuda.synchronize()
    return y, counts


# ------------------------------------------------------------------------------------------ one-shot
F32_HEAD = [c[0] for c in WR.F32_CASES]
#          member, samples, what the row starts with
ONE_SHOT = [(0, 1023, np.arange(256)), (0, 0, None), (1, 1023, np.arange(256)), (1, 1, None), (2, 1023, np.arange(256)), (2, 3, None),
            (3, 160, None), (3, 5, None), (4, 161, F32_HEAD), (4, 1023, None), (5, 4, None), (5, 161, None), (6, 1023, None),
            (6, 159, None)]


@pytest.fixture(scope="module")
def one_shot():
    assert len(ONE_SHOT) == 14 and sorted(set(n for _, n, _ in ONE_SHOT)) == [0, 1, 3, 4, 5, 159, 160, 161, 1023]
    assert sorted(m for m, _, _ in ONE_SHOT) == sorted(2 * list(range(len(BANK))))
    rng = np.random.default_rng(711)
    members = [m for m, _, _ in ONE_SHOT]
    raws = [raw_signal(rng, BANK[m][1], n, head) for m, n, head in ONE_SHOT]
    want = {dt: oracle_one_shot(dt, raws, members) for dt in OUT}
    # control: the mu-law rows read as A-law are another signal, so a decoder that ignored the encoding could not pass
    as_alaw = [1 if m == 0 else m for m in members]
    other = {dt: oracle_one_shot(dt, raws, as_alaw) for dt in OUT}
    return dict(members=members, raws=raws, host=pack_rows(raws), want=want, other=other)


@pytest.mark.parametrize("grid", GRIDS, ids=["grid_default", "grid1", "grid2"])
@pytest.mark.parametrize("out_dtype", OUT, ids=["f32", "i16"])
def test_one_shot_rows_equal_the_int16_path_on_the_decoded_rows(one_shot, out_dtype, grid):
    members, host = one_shot["members"], one_shot["host"]
    lens = [n for _, n, _ in ONE_SHOT]
    bank = ResampleBank(BANK, NEW, out_dtype=out_dtype)
    cap_grid(bank, grid)
    got, counts = bank(torch.from_numpy(host).to(DEV), [BANK[m] for m in members], lengths=lens)
    torch.cuda.synchronize()
    y, want_counts = one_shot["want"][out_dtype]
    assert got.dtype == out_dtype and counts == want_counts
    for r, c in enumerate(counts):
        assert torch.equal(bits(got[r, :c]), bits(y[r, :c])), (out_dtype, grid, r, BANK[members[r]], lens[r])
        assert not got[r, c:].any(), f"row {r}: zeros past the count"
    # the control: row 0 (all 256 mu-law codes) is NOT what its bytes give as A-law
    z, zc = one_shot["other"][out_dtype]
    assert zc[0] == counts[0] and not torch.equal(bits(z[0, :zc[0]]), bits(y[0, :zc[0]]))
    assert not torch.equal(bits(got[0, :zc[0]]), bits(z[0, :zc[0]]))


def test_default_lengths_and_int16_rows_on_a_wire_bank(one_shot):
    """Without ``lengths`` a row is as full as its bytes allow; int16 and float tensors go where they always went and carry rows
    of s16 members only."""
    rng = np.random.default_rng(5)
    raws = [raw_signal(rng, "mulaw", 164), raw_signal(rng, "f32", 41), raw_signal(rng, "s16", 82)]
    members = [0, 4, 3]
    bank = ResampleBank(BANK, NEW, out_dtype=I16)
    got, counts = bank(torch.from_numpy(pack_rows(raws)).to(DEV), [BANK[m] for m in members])
    y, want = oracle_one_shot(I16, raws, members)
    assert counts == want
    for r, c in enumerate(counts):
        assert torch.equal(got[r, :c], y[r, :c])
    s = torch.from_numpy(np.stack([raws[2], raws[2][::-1].copy()])).to(DEV)
    a, ca = bank(s, [8000, (44100, "s16")])
    b, cb = ResampleBank(RATES, NEW, out_dtype=I16)(s, [8000, 44100])
    assert ca == cb and torch.equal(a, b)
    with pytest.raises(_capi.HipLibraryError, match="mulaw"):
        bank(s, [(8000, "mulaw"), 8000])
    with pytest.raises(ValueError, match="not in the bank"):
        bank(s, [(8000, "f32"), 8000])
    with pytest.raises(ValueError, match="not in the bank"):
        bank(s, [16000, 8000])                                   # 16000 is in the bank as mu-law only


def test_one_shot_refusals_write_nothing(one_shot):
    lib = _capi.load()
    members = np.asarray(one_shot["members"], dtype=np.int32)
    ns = np.asarray([n for _, n, _ in ONE_SHOT], dtype=np.int32)
    bank = ResampleBank(BANK, NEW)
    xd = torch.from_numpy(one_shot["host"]).to(DEV)
    B, row_bytes, mcap = int(xd.size(0)), int(xd.size(1)), 2100
    out = torch.full((B, mcap), 7.0, device=DEV)
    torch.cuda.synchronize()

    def call(ptr=None, rb=row_bytes, nsamp=ns, mem=members, cap=mcap):
        return lib.wekws_hip_resample_bank_compute_wire(bank._ptr, xd.data_ptr() if ptr is None else ptr, B, rb, nsamp.ctypes.data,
                                                        mem.ctypes.data, out.data_ptr(), cap, None)
    assert call(ptr=xd.data_ptr() + 2) == -1 and "aligned" in _capi.last_error()
    assert call(rb=row_bytes - 2) == -1 and "row_bytes" in _capi.last_error()
    long = ns.copy()
    long[9] = row_bytes // 4 + 1                                # the float32 row: one sample more than its bytes
    assert call(nsamp=long) == -1 and "row 9" in _capi.last_error() and "f32" in _capi.last_error()
    bad = members.copy()
    bad[3] = len(BANK)
    assert call(mem=bad) == -1 and "member" in _capi.last_error()
    assert call(cap=100) == -1 and "mcap" in _capi.last_error()
    # the int16 entry point on the wire bank: a row of a member that is not s16
    assert lib.wekws_hip_resample_bank_compute_i16(bank._ptr, xd.data_ptr(), B, 8, None, members.ctypes.data, out.data_ptr(), mcap,
                                                   None) == -1 and "_wire" in _capi.last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call writes nothing"
    assert call() == 0
    torch.cuda.synchronize()
    y, counts = one_shot["want"][F32]
    for r, c in enumerate(counts):
        assert torch.equal(bits(out[r, :c]), bits(y[r, :c])) and not out[r, c:].any()


# ------------------------------------------------------------------------------------------ streaming
NS = 8
STREAM_MEMBER = [0, 1, 2, 3, 4, 5, 6, 0]
SIG = 700
CHUNKS = [0, 1, 2, 3, 5, 160, 161]


def chunkings(rng):
    """Per stream, chunk sizes from CHUNKS that sum to SIG (the last one cut): small ones often, so that the seam between the
    kept samples and the chunk moves a byte at a time."""
    out = []
    for _ in range(NS):
        sizes, left = [], SIG
        while left > 0:
            n = min(int(rng.choice(CHUNKS, p=[0.1, 0.2, 0.15, 0.15, 0.15, 0.125, 0.125])), left)
            sizes.append(n)
            left -= n
        out.append(sizes)
    return out


@pytest.mark.parametrize("out_dtype", OUT, ids=["f32", "i16"])
def test_streams_equal_the_one_shot_result_and_the_int16_path_push_by_push(out_dtype):
    rng = np.random.default_rng(2711)
    raws = [raw_signal(rng, BANK[m][1], SIG, F32_HEAD if BANK[m][1] == "f32" else None) for m in STREAM_MEMBER]
    pcm = [WR.decode(BANK[m][1], a) for a, m in zip(raws, STREAM_MEMBER)]
    whole, whole_counts = oracle_one_shot(out_dtype, raws, STREAM_MEMBER)
    rs = StreamingResamplerBank(NS, BANK, NEW, max_chunk=161, out_dtype=out_dtype)
    ref = StreamingResamplerBank(NS, RATES, NEW, max_chunk=161, out_dtype=out_dtype)       # the int16 path, same chunks
    for m in sorted(set(STREAM_MEMBER)):
        ids = [s for s in range(NS) if STREAM_MEMBER[s] == m]
        rs.set_rate(ids, BANK[m])
        ref.set_rate(ids, BANK[m][0])
    assert [rs.encoding_of(s) for s in range(NS)] == [BANK[m][1] for m in STREAM_MEMBER]
    assert [rs.rate_of(s) for s in range(NS)] == [BANK[m][0] for m in STREAM_MEMBER]
    plan = chunkings(rng)
    at, nxt = [0] * NS, [0] * NS
    pieces = [[] for _ in range(NS)]
    pushes = 0
    while True:
        live = [s for s in range(NS) if nxt[s] < len(plan[s])]
        flush = not live
        ids = list(rng.permutation(NS)) if flush else [int(s) for s in rng.permutation(live)[:int(rng.integers(1, len(live) + 1))]]
        ns = [0 if flush else plan[s][nxt[s]] for s in ids]
        wire = torch.from_numpy(pack_rows([raws[s][at[s]:at[s] + n] for s, n in zip(ids, ns)])).to(DEV)
        x16 = np.full((len(ids), max(ns + [1])), 12345, dtype=np.int16)
        for i, (s, n) in enumerate(zip(ids, ns)):
            x16[i, :n] = pcm[s][at[s]:at[s] + n]
        got, counts = rs.push(wire, samples=ns, streams=ids, flush=flush)
        exp, exp_counts = ref.push(torch.from_numpy(x16).to(DEV), samples=ns, streams=ids, flush=flush)
        assert counts == exp_counts and torch.equal(bits(got), bits(exp)), (pushes, ids, ns)
        for i, (s, n) in enumerate(zip(ids, ns)):
            pieces[s].append(got[i, :counts[i]])
            at[s] += n
            if not flush:
                nxt[s] += 1
            assert rs.counts(s) == ref.counts(s)
        pushes += 1
        if flush:
            break
    assert at == [SIG] * NS and pushes > 20
    for s in range(NS):
        y = torch.cat(pieces[s])
        assert y.numel() == whole_counts[s] == rs.counts(s)[1]
        assert torch.equal(bits(y), bits(whole[s, :whole_counts[s]])), (out_dtype, s, BANK[STREAM_MEMBER[s]])
        assert rs.counts(s) == (SIG, whole_counts[s], 0, 1)


def test_set_rate_between_two_encodings_of_one_rate_restarts_the_named_streams():
    rng = np.random.default_rng(99)
    first = [raw_signal(rng, "mulaw", 160) for _ in range(4)]
    second = [raw_signal(rng, "mulaw", 161) for _ in range(4)]
    rs = StreamingResamplerBank(4, BANK, NEW, max_chunk=161, out_dtype=I16)
    a, ca = rs.push(torch.from_numpy(pack_rows(first)).to(DEV), samples=[160] * 4)
    before = [rs.counts(s) for s in range(4)]
    rs.set_rate([2, 1], (8000, "alaw"))
    assert [rs.encoding_of(s) for s in range(4)] == ["mulaw", "alaw", "alaw", "mulaw"] and [rs.rate_of(s) for s in range(4)] == [8000] * 4
    assert [rs.counts(s) for s in range(4)] == [before[0], (0, 0, 0, 0), (0, 0, 0, 0), before[3]]
    with pytest.raises(ValueError, match="not in the bank"):
        rs.set_rate([0], (8000, "f32"))
    with pytest.raises(_capi.HipLibraryError, match="outside"):
        rs.set_rate([0, 4], (8000, "alaw"))
    assert rs.encoding_of(0) == "mulaw"
    b, cb = rs.push(torch.from_numpy(pack_rows(second)).to(DEV), samples=[161] * 4, flush=True)
    # streams 1 and 2: a fresh A-law stream of the second chunk alone; 0 and 3: their mu-law signal continued
    members = [0, 1, 1, 0]
    whole = [np.concatenate([first[s], second[s]]) if members[s] == 0 else second[s] for s in range(4)]
    y, counts = oracle_one_shot(I16, whole, members)
    for s in range(4):
        got = torch.cat([a[s, :ca[s]], b[s, :cb[s]]]) if members[s] == 0 else b[s, :cb[s]]
        assert got.numel() == counts[s] and torch.equal(got, y[s, :counts[s]]), s
    rs.set_rate(None, 44100)
    assert {rs.encoding_of(s) for s in range(4)} == {"s16"} and {rs.rate_of(s) for s in range(4)} == {44100}


def test_refused_pushes_change_no_stream_and_write_nothing():
    lib = _capi.load()
    rng = np.random.default_rng(3)
    rs = StreamingResamplerBank(4, BANK, NEW, max_chunk=161, out_dtype=F32)
    rs.set_rate([1], (48000, "f32"))
    rs.set_rate([2], 8000)
    raws = [raw_signal(rng, e, 160) for e in ("mulaw", "f32", "s16", "mulaw")]
    rs.push(torch.from_numpy(pack_rows(raws)).to(DEV), samples=[160] * 4)
    before = [rs.counts(s) for s in range(4)]
    wire = torch.from_numpy(pack_rows(raws, 640)).to(DEV)
    ids = np.arange(4, dtype=np.int32)
    cap = rs.max_out(161)
    out = torch.full((4, cap), 7.0, device=DEV)
    got = np.zeros(4, dtype=np.int32)
    torch.cuda.synchronize()

    def push_wire(ns, ptr=None, rb=640, which=ids):
        ns = np.asarray(ns, dtype=np.int32)
        return lib.wekws_hip_resample_bank_push_wire(rs._ptr, wire.data_ptr() if ptr is None else ptr, len(ns), rb, which.ctypes.data,
                                                     ns.ctypes.data, 0, out.data_ptr(), cap, got.ctypes.data, None)
    assert push_wire([160, 161, 160, 160]) == -1 and "row 1" in _capi.last_error()          # 161 floats are 644 bytes
    assert push_wire([160, 40, 160, 160], rb=160) == -1 and "row 2" in _capi.last_error()   # 160 int16 samples are 320 bytes
    assert push_wire([162, 1, 1, 1]) == -1 and "row 0" in _capi.last_error()                # max_chunk counts samples
    assert push_wire([1, 1, 1, 1], ptr=wire.data_ptr() + 1) == -1 and "aligned" in _capi.last_error()
    assert push_wire([1, 1, 1, 1], rb=642) == -1 and "row_bytes" in _capi.last_error()
    assert push_wire([1, 1], which=np.asarray([3, 3], dtype=np.int32)) == -1 and "twice" in _capi.last_error()
    # the int16 push: a row of a mu-law stream is refused, whatever the other rows are
    x16 = torch.zeros((4, 160), dtype=torch.int16, device=DEV)
    ns = np.full(4, 160, dtype=np.int32)
    order = np.asarray([2, 0, 1, 3], dtype=np.int32)
    assert lib.wekws_hip_resample_bank_push(rs._ptr, x16.data_ptr(), 4, 160, order.ctypes.data, ns.ctypes.data, 0, out.data_ptr(), cap,
                                            got.ctypes.data, None) == -1
    assert "row 1" in _capi.last_error() and "mulaw" in _capi.last_error()
    with pytest.raises(_capi.HipLibraryError, match="_wire"):
        rs.push(x16[:2], streams=[2, 0])
    torch.cuda.synchronize()
    assert [rs.counts(s) for s in range(4)] == before and bool((out == 7.0).all()) and not got.any()
    # ... and the s16 stream alone is served by the int16 push, as ever
    y, c = rs.push(x16[:1], streams=[2])
    assert c[0] > 0 and rs.counts(2)[0] == 320 and [rs.counts(s) for s in (0, 1, 3)] == [before[0], before[1], before[3]]
    assert push_wire([160, 160, 160, 160]) == 0 and got.min() > 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).all())


def test_a_list_of_bytes_is_read_per_stream():
    rng = np.random.default_rng(17)
    ids = [5, 0, 4, 3, 2]
    a = StreamingResamplerBank(NS, BANK, NEW, max_chunk=161, out_dtype=I16)
    b = StreamingResamplerBank(NS, BANK, NEW, max_chunk=161, out_dtype=I16)
    for rs in (a, b):
        for s in range(NS):
            rs.set_rate([s], BANK[STREAM_MEMBER[s]])
    for n, flush in ((161, False), (37, False), (5, True)):
        lens = [n, max(n - 3, 0), n, 1, 0]
        raws = [raw_signal(rng, BANK[STREAM_MEMBER[s]][1], k) for s, k in zip(ids, lens)]
        # bytes (a trailing partial sample is dropped), or arrays of the encoding's own dtype
        chunks = [r.tobytes() + (b"\x01" if r.dtype.itemsize > 1 else b"") if i % 2 == 0 else r for i, r in enumerate(raws)]
        y1, c1 = a.push(chunks, streams=ids, flush=flush)
        y2, c2 = b.push(torch.from_numpy(pack_rows(raws)).to(DEV), samples=lens, streams=ids, flush=flush)
        assert c1 == c2 and torch.equal(y1, y2)
        assert [a.counts(s) for s in ids] == [b.counts(s) for s in ids]
    a.reset()
    with pytest.raises(ValueError, match="float32"):
        a.push([np.zeros(4, dtype=np.int16)], streams=[4])
    assert ENCODINGS == WR.ENCODINGS
