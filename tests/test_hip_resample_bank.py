"""GPU: the rate bank (wekws_hip_resample_bank_*: wekws_amd.frontend.ResampleBank / StreamingResamplerBank) -- rows and streams of
different source rates in one launch -- against the single-rate resampler of every row's rate, bit for bit.

No tolerance of its own: a row of member m equals Resample(rate_m) / StreamingResampler(rate_m) on the same samples exactly
(integer views), and where the float64 restatement is asked directly the bar is the resampler's derived one,
(live_i + 2) 2^-24 sum |k||x| (tests/test_hip_resample.py).  A grid capped to 1 or 3 workgroups (a hook of the test library) makes
one workgroup walk tiles of several members, so the table reload is on every such run's path."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import resample_ref as RR
from tests.test_hip_resample import (HOOKS, TILE, assert_queued_calls_equal_synchronised_ones, one_shot_rows, plan, within_bar,
                                     within_bar_i16)
from wekws_amd import _capi
from wekws_amd.frontend import Resample, ResampleBank, StreamingResampler, StreamingResamplerBank

pytestmark = pytest.mark.gpu

DEV = "cuda"
BANK = (48000, 8000, 44100, 24000, 16000)
NEW = 16000
GRIDS = [1, 3, None]
F32, I16 = torch.float32, torch.int16


def hooks_lib():
    lib = C.CDLL(HOOKS)
    lib.wekws_hip_debug_resample_bank_set_grid.restype = C.c_int
    lib.wekws_hip_debug_resample_bank_set_grid.argtypes = [C.c_void_p, C.c_int]
    lib.wekws_hip_debug_resample_bank_round_taps_f16.restype = C.c_int
    lib.wekws_hip_debug_resample_bank_round_taps_f16.argtypes = [C.c_void_p, C.c_int]
    return lib


def cap_grid(handle, grid):
    assert hooks_lib().wekws_hip_debug_resample_bank_set_grid(handle._ptr, grid or 0) == 0


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------------------------------ one-shot
ROWS = 6          # of one_shot_rows: lengths 0, 1, o - 1, K, 3 tiles' input + 1, 3 tiles' input - 1


@pytest.fixture(scope="module")
def mixed():
    """The mixed batch -- row r is row r // 5 of member r % 5, so neighbouring rows differ in member -- and, computed once,
    every member's rows through the single-rate kernel for each input / output type."""
    per = [one_shot_rows(plan(r, NEW)) for r in BANK]
    width = max(x.shape[1] for x, _ in per)
    B = ROWS * len(BANK)
    x = np.full((B, width), 12345, dtype=np.int16)               # past a row's length: must not be read as signal
    lens, rates = [], []
    for r in range(B):
        m, k = r % len(BANK), r // len(BANK)
        xm, lm = per[m]
        x[r, :xm.shape[1]] = xm[k]
        lens.append(lm[k])
        rates.append(BANK[m])
    want = {}
    for in_dt in (I16, F32):
        for out_dt in (F32, I16):
            for m, rate in enumerate(BANK):
                xm, lm = per[m]
                y, counts = Resample(rate, NEW, out_dtype=out_dt)(torch.from_numpy(xm[:ROWS]).to(DEV).to(in_dt), lengths=lm[:ROWS])
                want[(in_dt, out_dt, m)] = (y, counts)
    torch.cuda.synchronize()
    return dict(x=x, lens=lens, rates=rates, want=want)


@pytest.mark.parametrize("grid", GRIDS, ids=["grid1", "grid3", "grid_default"])
def test_mixed_batch_equals_the_single_rate_kernel_row_by_row(mixed, grid):
    x, lens, rates = mixed["x"], mixed["lens"], mixed["rates"]
    for in_dt in (I16, F32):
        xd = torch.from_numpy(x).to(DEV).to(in_dt)
        for out_dt in (F32, I16):
            bank = ResampleBank(BANK, NEW, out_dtype=out_dt)
            cap_grid(bank, grid)
            got, counts = bank(xd, rates, lengths=lens)
            assert got.dtype == out_dt and got.size(0) == len(lens)
            assert counts == [plan(r, NEW).num_samples(n) for r, n in zip(rates, lens)]
            for r in range(len(lens)):
                m, k = r % len(BANK), r // len(BANK)
                y, c = mixed["want"][(in_dt, out_dt, m)]
                assert c[k] == counts[r]
                assert torch.equal(bits(got[r, :counts[r]]), bits(y[k, :counts[r]])), (in_dt, out_dt, grid, r, rates[r])
                assert not got[r, counts[r]:].any(), f"row {r}: zeros past the count"
            if in_dt == I16 and out_dt == F32:
                # one row per member straight to the float64 oracle's bar
                g = got.cpu().numpy()
                for m, rate in enumerate(BANK):
                    r = 4 * len(BANK) + m
                    within_bar(plan(rate, NEW), g[r, :counts[r]], x[r, :lens[r]], f"bank row {r} ({rate}, len {lens[r]}, grid {grid})")


def test_one_shot_refusals_write_nothing(mixed):
    lib = _capi.load()
    x, lens, rates = mixed["x"], mixed["lens"], mixed["rates"]
    B = len(lens)
    bank = ResampleBank(BANK, NEW)
    xd = torch.from_numpy(x).to(DEV)
    with pytest.raises(ValueError, match="not in the bank"):
        bank(xd, [22050] + rates[1:], lengths=lens)
    ns = np.asarray(lens, dtype=np.int32)
    members = np.asarray([BANK.index(r) for r in rates], dtype=np.int32)
    mcap = max(plan(r, NEW).num_samples(n) for r, n in zip(rates, lens))
    out = torch.full((B, mcap), 7.0, device=DEV)
    torch.cuda.synchronize()
    for bad in (len(BANK), -1):
        mem = members.copy()
        mem[B - 3] = bad
        rc = lib.wekws_hip_resample_bank_compute_i16(bank._ptr, xd.data_ptr(), B, x.shape[1], ns.ctypes.data, mem.ctypes.data,
                                                     out.data_ptr(), mcap, None)
        assert rc == -1 and "member" in _capi.last_error()
    rc = lib.wekws_hip_resample_bank_compute_i16(bank._ptr, xd.data_ptr(), B, x.shape[1], ns.ctypes.data, members.ctypes.data,
                                                 out.data_ptr(), mcap - 1, None)
    assert rc == -1 and "mcap" in _capi.last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call writes nothing"
    # ... and the same call with room is served
    rc = lib.wekws_hip_resample_bank_compute_i16(bank._ptr, xd.data_ptr(), B, x.shape[1], ns.ctypes.data, members.ctypes.data,
                                                 out.data_ptr(), mcap, None)
    torch.cuda.synchronize()
    assert rc == 0 and not bool((out == 7.0).any())


# ------------------------------------------------------------------------------------------ non-finite
def test_non_finite_rows_follow_the_full_window_of_their_member():
    """A NaN, a +Inf and a -Inf in one row per member, once under a live tap of an output and once inside its K-tap window under a
    tap the clamp zeroes (the copy member has a single live tap and no clamped one: live only).  Classes as the full-window
    convolution gives them; every other row of the batch bit-identical to the clean run."""
    rng = np.random.default_rng(11)
    plans = [plan(r, NEW) for r in BANK]
    L = [3 * -(-TILE * p.o // p.n) + 50 for p in plans]
    width = max(L)
    clean = np.zeros((2 * len(BANK), width), dtype=np.float32)
    rates, lens, spots = [], [], []
    for m, p in enumerate(plans):
        for k in (0, 1):                                           # row 2m takes the value, row 2m + 1 stays clean
            clean[2 * m + k, :L[m]] = rng.uniform(-3e4, 3e4, L[m])
            rates.append(BANK[m])
            lens.append(L[m])
        j, i = 3 + 200 // p.o, min(5, p.n - 1)
        live_pos = j * p.o + int(p.first[i]) + min(4, int(p.last[i] - p.first[i])) - p.width
        dead_tap = p.K - 1 if p.last[i] < p.K - 1 else (0 if p.first[i] > 0 else None)
        dead_pos = None if dead_tap is None else j * p.o + dead_tap - p.width
        assert 0 <= live_pos < L[m] and (dead_pos is None or (0 <= dead_pos < L[m] and not p.live[i, dead_tap] and p.taps[i, dead_tap] == 0))
        assert (dead_pos is None) == (BANK[m] == NEW)
        spots.append((j * p.n + i, live_pos, dead_pos))
    bank = ResampleBank(BANK, NEW)
    cap_grid(bank, 3)
    base, counts = bank(torch.from_numpy(clean).to(DEV), rates, lengths=lens)
    base = base.cpu().numpy()
    for val in (np.nan, np.inf, -np.inf):
        for kind in (1, 2):
            x = clean.copy()
            for m, s in enumerate(spots):
                if s[kind] is not None:
                    x[2 * m, s[kind]] = val
            got = bank(torch.from_numpy(x).to(DEV), rates, lengths=lens)[0].cpu().numpy()
            for m, p in enumerate(plans):
                a, b, c = 2 * m, 2 * m + 1, counts[2 * m]
                assert np.array_equal(got[b].view(np.int32), base[b].view(np.int32)), (val, kind, BANK[m])
                if spots[m][kind] is None:
                    assert np.array_equal(got[a].view(np.int32), base[a].view(np.int32))
                    continue
                want_cls = RR.classes(p, x[a, :L[m]])
                assert np.array_equal(RR.classify(got[a, :c]), want_cls), (val, kind, BANK[m])
                assert want_cls[spots[m][0]] != 0 and (want_cls != 0).sum() >= min(p.n, 2)
                want, mag = RR.resample(p, x[a, :L[m]])
                fin = want_cls == 0
                assert fin.sum() > 100 and (np.abs(got[a, :c][fin] - want[fin]) <= RR.bar(p, mag)[fin]).all(), (val, kind, BANK[m])
                assert not got[a, c:].any()


# ------------------------------------------------------------------------------------------ streaming
NS, SIG = 12, 3000


def member_of(s):
    return s % len(BANK)


def schedule(seed):
    """pushes: per push a list of (stream, n) -- subsets of the streams in shuffled order, different lengths per row, zero-length
    chunks among them; the last push names every stream with what is left of it (possibly nothing) and is the flush"""
    rng = np.random.default_rng(seed)
    left = [SIG] * NS
    pushes = []
    while sum(left) > NS * SIG // 4:
        pick = [s for s in range(NS) if rng.random() < 0.7] or [0]
        pick = [pick[i] for i in rng.permutation(len(pick))]
        push = []
        for s in pick:
            n = min(int(rng.choice([0, 1, 17, 160, 441, 997, 1200])), left[s])
            left[s] -= n
            push.append((s, n))
        pushes.append(push)
    pushes.append([(s, left[s]) for s in rng.permutation(NS).tolist()])
    return pushes


def run_schedule(rs, sig, pushes, pos=None, on_push=None):
    """Feeds the pushes (the last one flushed); returns per stream the list of its outputs, and the counts of every push."""
    pos = [0] * NS if pos is None else pos
    outs = [[] for _ in range(NS)]
    all_counts = []
    for k, push in enumerate(pushes):
        if on_push is not None:
            on_push(k)
        ids = [s for s, _ in push]
        chunks = []
        for s, n in push:
            chunks.append(sig[s, pos[s]:pos[s] + n])
            pos[s] += n
        out, counts = rs.push(chunks, streams=ids, flush=(k == len(pushes) - 1))
        for b, s in enumerate(ids):
            assert not out[b, counts[b]:].any()
            outs[s].append(out[b, :counts[b]])
        all_counts.append(counts)
    return outs, all_counts


@pytest.fixture(scope="module")
def streams():
    """The signals, five seeded schedules, and -- computed once -- what the single-rate resamplers say: the counts of every push
    from a StreamingResampler of each rate fed the same chunks, the whole signals through the one-shot kernel per output type."""
    rng = np.random.default_rng(77)
    sig = rng.integers(-32768, 32768, (NS, SIG), dtype=np.int16)
    scheds = [schedule(100 + k) for k in range(5)]
    assert all(any(n == 0 for p in sc for _, n in p) and len({len(p) for p in sc}) > 1 for sc in scheds)
    singles = [StreamingResampler(NS, r, NEW, max_chunk=SIG) for r in BANK]
    ref_counts = []
    for sc in scheds:
        for rs in singles:
            rs.reset()
        pos = [0] * NS
        per_push = []
        for k, push in enumerate(sc):
            want = {}
            for m, rs in enumerate(singles):
                part = [(s, n) for s, n in push if member_of(s) == m]
                if not part:
                    continue
                _, counts = rs.push([sig[s, pos[s]:pos[s] + n] for s, n in part], streams=[s for s, _ in part], flush=(k == len(sc) - 1))
                want.update({s: c for (s, _), c in zip(part, counts)})
            for s, n in push:
                pos[s] += n
            per_push.append([want[s] for s, _ in push])
        ref_counts.append(per_push)
    whole = {}
    for dt in (F32, I16):
        for s in range(NS):
            whole[(dt, s)] = Resample(BANK[member_of(s)], NEW, out_dtype=dt)(torch.from_numpy(sig[s:s + 1]).to(DEV))[0]
    torch.cuda.synchronize()
    return dict(sig=sig, scheds=scheds, ref_counts=ref_counts, whole=whole)


def make_streaming_bank(out_dtype, grid):
    rs = StreamingResamplerBank(NS, BANK, NEW, max_chunk=SIG, out_dtype=out_dtype)
    cap_grid(rs, grid)
    for m, rate in enumerate(BANK):
        rs.set_rate([s for s in range(NS) if member_of(s) == m], rate)
    assert [rs.rate_of(s) for s in range(NS)] == [BANK[member_of(s)] for s in range(NS)]
    return rs


@pytest.mark.parametrize("grid", [1, None], ids=["grid1", "grid_default"])
@pytest.mark.parametrize("out_dtype", [F32, I16], ids=["f32", "i16"])
def test_streams_of_mixed_rates_equal_the_one_shot_kernel_bit_for_bit(streams, out_dtype, grid):
    rs = make_streaming_bank(out_dtype, grid)
    for k, sc in enumerate(streams["scheds"]):
        rs.reset()
        outs, counts = run_schedule(rs, streams["sig"], sc)
        assert counts == streams["ref_counts"][k], f"schedule {k}: counts of every push"
        for s in range(NS):
            got, want = torch.cat(outs[s]), streams["whole"][(out_dtype, s)]
            assert got.dtype == out_dtype and torch.equal(bits(got), bits(want)), (k, s, BANK[member_of(s)])
            assert rs.counts(s) == (SIG, want.numel(), 0, 1)


def test_set_rate_restarts_the_streams_it_names(streams):
    sig, sc = streams["sig"], streams["scheds"][1]
    at = len(sc) // 2
    moved = {3: 48000, 7: 16000}                                   # from 24000 and from 44100
    assert all(BANK[member_of(s)] != r for s, r in moved.items())
    plain, _ = run_schedule(make_streaming_bank(I16, None), sig, sc)
    rs = make_streaming_bank(I16, 1)
    start = {}

    def change(k):
        if k == at:
            before = [rs.counts(s) for s in range(NS)]
            assert any(c[0] > 0 for c in before)
            # refusals: a rate outside the bank, a bad stream behind good ones, a bad member -- nothing changes
            with pytest.raises(ValueError, match="not in the bank"):
                rs.set_rate([3], 22050)
            with pytest.raises(_capi.HipLibraryError, match="outside"):
                rs.set_rate([3, 7, NS], 48000)
            ids = (C.c_int32 * 2)(3, 7)
            assert _capi.load().wekws_hip_resample_bank_set_rate(rs._ptr, ids, 2, len(BANK)) == -1 and "member" in _capi.last_error()
            with pytest.raises(_capi.HipLibraryError, match="outside"):
                rs.rate_of(NS)
            assert [rs.counts(s) for s in range(NS)] == before
            assert [rs.rate_of(s) for s in range(NS)] == [BANK[member_of(s)] for s in range(NS)]
            for s, rate in moved.items():
                rs.set_rate([s], rate)
                assert rs.rate_of(s) == rate and rs.counts(s) == (0, 0, 0, 0)
                start[s] = before[s][0]
            assert [rs.counts(s) for s in range(NS) if s not in moved] == [before[s] for s in range(NS) if s not in moved]

    outs, _ = run_schedule(rs, sig, sc, on_push=change)
    for s in range(NS):
        if s not in moved:
            assert len(outs[s]) == len(plain[s]) and all(torch.equal(a, b) for a, b in zip(outs[s], plain[s])), s
    for s, rate in moved.items():
        pushes_before = sum(1 for push in sc[:at] for t, _ in push if t == s)
        after = torch.cat(outs[s][pushes_before:])
        fresh = Resample(rate, NEW, out_dtype=I16)(torch.from_numpy(sig[s:s + 1, start[s]:].copy()).to(DEV))[0]
        assert 0 < start[s] < SIG and torch.equal(after, fresh), (s, rate)
        assert rs.counts(s) == (SIG - start[s], fresh.numel(), 0, 1)
    # a push after the flush is refused until the stream is reset
    chunk = torch.zeros((1, 100), dtype=torch.int16, device=DEV)
    with pytest.raises(_capi.HipLibraryError, match="flushed"):
        rs.push(chunk, streams=[3])
    assert rs.counts(3)[3] == 1
    rs.reset([3])
    out, counts = rs.push(chunk, streams=[3])
    assert rs.rate_of(3) == 48000 and counts[0] == plan(48000, NEW).step(0, 100, False)[0] and not out.any()


def test_one_shot_calls_and_pushes_share_one_ring():
    """tests/test_hip_resample.py's test of the same name on a bank: the one-shot rows are of mixed members (so every table is
    sorted on its way into the ring), the three streams one per member"""
    lib = _capi.load()
    rates = (8000, 44100, 48000)

    def make():
        rs = StreamingResamplerBank(3, rates, NEW, max_chunk=600)
        for s, rate in enumerate(rates):
            rs.set_rate([s], rate)
        return rs

    def one_shot(rs, x):
        B, n = int(x.size(0)), int(x.size(1))
        members = np.asarray([(2 * b + B) % 3 for b in range(B)], dtype=np.int32)
        m = max(int(lib.wekws_hip_resample_num_samples(r, NEW, n)) for r in rates)
        out = torch.empty((B, m), dtype=torch.int16, device=DEV)
        _capi.check(lib.wekws_hip_resample_bank_compute_i16(rs._ptr, x.data_ptr(), B, n, None, members.ctypes.data, out.data_ptr(), m,
                                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "bank compute_i16")
        return out

    xs, queued = assert_queued_calls_equal_synchronised_ones(make, one_shot)
    B = int(xs[8].size(0))
    for b in (0, 4, 5):                                             # B = 6: members 0, 2, 1
        p = plan(rates[(2 * b + B) % 3], NEW)
        within_bar_i16(p, queued[8][b, :p.num_samples(3000)].cpu().numpy(), xs[8][b].cpu().numpy(), f"queued call 8 row {b}")
        assert not queued[8][b, p.num_samples(3000):].any()


# ------------------------------------------------------------------------------------------ negative control
def test_fp16_taps_of_one_member_miss_the_bar_for_its_rows_alone(mixed):
    x, lens, rates = mixed["x"], mixed["lens"], mixed["rates"]
    xd = torch.from_numpy(x).to(DEV)
    bank = ResampleBank(BANK, NEW)
    clean, counts = bank(xd, rates, lengths=lens)
    torch.cuda.synchronize()
    hooks = hooks_lib()
    assert hooks.wekws_hip_debug_resample_bank_round_taps_f16(bank._ptr, len(BANK)) == -1
    assert hooks.wekws_hip_debug_resample_bank_round_taps_f16(bank._ptr, BANK.index(44100)) == 0
    got, _ = bank(xd, rates, lengths=lens)
    torch.cuda.synchronize()
    del bank                                                        # (there is no way back from the rounding)
    p = plan(44100, NEW)
    for r in range(len(lens)):
        if rates[r] != 44100:
            assert torch.equal(bits(got[r]), bits(clean[r])), (r, rates[r])
    r = 4 * len(BANK) + BANK.index(44100)
    want, mag = RR.resample(p, x[r, :lens[r]])
    ratio = np.abs(got[r, :counts[r]].cpu().numpy() - want) / RR.bar(p, mag)
    miss = float((ratio > 1).mean())
    print(f"bank member 44100: fp16 taps miss the bar at {miss:.1%} of the outputs, by up to {ratio.max():.0f}x")
    assert miss > 0.5


# ------------------------------------------------------------------------------------------ scale
def test_4096_streams_of_three_rates_in_one_push():
    rates, chunk = (8000, 16000, 48000), {8000: 800, 16000: 1600, 48000: 4800}
    cuts = [0, 1365, 2730, 4096]
    g = torch.Generator(device="cpu").manual_seed(5)
    xd = torch.randint(-32768, 32768, (4096, 4800), dtype=torch.int16, generator=g).to(DEV)
    samples = [chunk[rates[m]] for m in range(3) for _ in range(cuts[m], cuts[m + 1])]
    for dt in (F32, I16):
        rs = StreamingResamplerBank(4096, rates, NEW, max_chunk=4800, out_dtype=dt)
        for m, rate in enumerate(rates):
            rs.set_rate(range(cuts[m], cuts[m + 1]), rate)
        out, counts = rs.push(xd, samples=samples, flush=True)
        assert counts == [1600] * 4096 and tuple(out.shape) == (4096, 1600)
        for m, rate in enumerate(rates):
            a, b = cuts[m], cuts[m + 1]
            one = StreamingResampler(b - a, rate, NEW, max_chunk=4800, out_dtype=dt)
            want, wc = one.push(xd[a:b, :chunk[rate]].contiguous(), flush=True)
            assert wc == counts[a:b] and torch.equal(bits(out[a:b]), bits(want)), (dt, rate)
