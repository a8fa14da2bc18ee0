"""GPU: the resampler (wekws_hip_resample_*: wekws_amd.frontend.Resample / StreamingResampler) against the float64 restatement
of torchaudio's Resample (tests/resample_ref.py).

The bar of output q with phase i is (live_i + 2) 2^-24 sum_m |k[i][m]| |x[..]|: the forward error bound of a live_i-term float32
accumulation plus one rounding of each tap -- derived, not tuned; where it is 0 the output must be exactly 0.  The oracle uses
the taps rounded to float32, as the reference's convolution does.  Streaming is held to the one-shot kernel bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import resample_ref as RR
from wekws_amd import _capi
from wekws_amd.frontend import Resample, StreamingResampler

pytestmark = pytest.mark.gpu

DEV = "cuda"
_PLANS = {}
HOOKS = os.path.join(os.path.dirname(_capi.lib_path()), "libwekws_hip_hooks.so")


def kernel_tile():
    """outputs of a workgroup's tile (kResampleTile), as the plan hook of the hooks library reports it"""
    hooks = C.CDLL(HOOKS)
    hooks.wekws_hip_debug_resample_plan.restype = C.c_int
    hooks.wekws_hip_debug_resample_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                    C.c_void_p, C.c_int64]
    dims = np.zeros(10, dtype=np.int64)
    assert hooks.wekws_hip_debug_resample_plan(48000, 16000, 6, 0.99, dims.ctypes.data, None, 0, None, None, 0) == 0
    assert int(dims[9]) > 0
    return int(dims[9])


TILE = kernel_tile()


def plan(orig, new):
    if (orig, new) not in _PLANS:
        _PLANS[(orig, new)] = RR.Plan(orig, new)
    return _PLANS[(orig, new)]


def within_bar(p, got, x, what):
    """got (count) against the oracle of the row x; returns the worst error in units of the bar"""
    want, mag = RR.resample(p, x)
    bar = RR.bar(p, mag)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want)
    assert (got[bar == 0] == 0).all(), what
    worst = float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0
    print(f"{what}: worst error {worst:.3f} of the bar")
    assert (err <= bar).all(), (what, worst)
    return worst


def one_shot_rows(p):
    """lengths {0, 1, o - 1, K, 3 tiles + 1, 3 tiles - 1} with random content, then a row of alternating +-32767 and an all-zero
    row of the long lengths: both ends and two tile seams are crossed"""
    rng = np.random.default_rng(p.orig)
    tile_in = -(-TILE * p.o // p.n)
    lens = [0, 1, p.o - 1, p.K, 3 * tile_in + 1, 3 * tile_in - 1, 3 * tile_in + 1, 3 * tile_in - 1]
    x = np.zeros((len(lens), max(lens) + 5), dtype=np.int16)
    for b, n in enumerate(lens[:6]):
        x[b, :n] = rng.integers(-32768, 32768, n)
        x[b, n:] = 12345                                  # past a row's length: must not be read as signal
    x[6, :lens[6]] = np.where(np.arange(lens[6]) % 2 == 0, 32767, -32767)
    return x, lens


@pytest.mark.parametrize("orig,new", RR.PAIRS)
def test_one_shot_within_the_bar(orig, new):
    p = plan(orig, new)
    x, lens = one_shot_rows(p)
    rs = Resample(orig, new)
    xi = torch.from_numpy(x).to(DEV)
    yi, counts = rs(xi, lengths=lens)
    yf, counts_f = rs(xi.to(torch.float32), lengths=lens)
    assert counts == counts_f == [p.num_samples(n) for n in lens]
    assert yi.dtype == torch.float32 and tuple(yi.shape) == (len(lens), p.num_samples(x.shape[1]))
    # float-out of int16 input == float-out of the widened input, bit for bit
    assert torch.equal(yi.view(torch.int32), yf.view(torch.int32))
    got = yi.cpu().numpy()
    for b, n in enumerate(lens):
        assert (got[b, counts[b]:] == 0).all(), f"row {b}: zeros past the count"
        within_bar(p, got[b, :counts[b]], x[b, :n], f"{orig}->{new} row {b} (len {n})")
    assert (got[7] == 0).all()
    # without lengths every row is nmax long
    y_all = rs(xi[4:5]).cpu().numpy()
    within_bar(p, y_all[0], x[4], f"{orig}->{new} whole row")
    # a capacity too small for a row is refused
    lib = _capi.load()
    ns = np.asarray(lens, dtype=np.int32)
    out = torch.zeros((len(lens), 4), device=DEV)
    rc = lib.wekws_hip_resample_compute_i16(rs._ptr, xi.data_ptr(), len(lens), x.shape[1], ns.ctypes.data, out.data_ptr(), 4, None)
    assert rc == -1 and "mcap" in _capi.last_error()


def test_one_shot_calls_queue_without_a_synchronise():
    """ten calls back to back -- more than the ring of row tables holds, with row counts that make slots grow -- equal the same
    calls made one at a time"""
    rs = Resample(44100, 16000)
    g = torch.Generator(device="cpu").manual_seed(3)
    xs = [torch.randint(-32768, 32768, (1 + (5 * k) % 7, 3000), dtype=torch.int16, generator=g).to(DEV) for k in range(10)]
    lens = [[3000 - 97 * b - k for b in range(x.size(0))] for k, x in enumerate(xs)]
    torch.cuda.synchronize()
    queued = [rs(x, lengths=n)[0] for x, n in zip(xs, lens)]
    torch.cuda.synchronize()
    for x, n, q in zip(xs, lens, queued):
        one = rs(x, lengths=n)[0]
        torch.cuda.synchronize()
        assert torch.equal(q.view(torch.int32), one.view(torch.int32))
    p = plan(44100, 16000)
    within_bar(p, queued[9][1, :p.num_samples(lens[9][1])].cpu().numpy(), xs[9][1, :lens[9][1]].cpu().numpy(), "queued call 9 row 1")


def alternate_one_shot_and_push(make, one_shot, rows, synchronise):
    """Ten calls on ONE handle of 3 streams (make()), alternately a one-shot call -- call k has 1 + (5 k mod 7) rows of 3000 samples,
    more than a table made for 3 streams holds -- and a push of 500 samples per stream.  one_shot(rs, x) -> out.  Returns every call's
    output, the pushes' counts and the streams' counts at the end."""
    rs = make()
    g = torch.Generator(device="cpu").manual_seed(11)
    xs = [torch.randint(-32768, 32768, (rows(k), 3000) if k % 2 == 0 else (3, 500), dtype=torch.int16, generator=g).to(DEV)
          for k in range(10)]
    torch.cuda.synchronize()
    outs, counts = [], []
    for k, x in enumerate(xs):
        if k % 2 == 0:
            outs.append(one_shot(rs, x))
        else:
            y, c = rs.push(x)
            outs.append(y)
            counts.append(c)
        if synchronise:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return xs, outs, counts, [rs.counts(s) for s in range(3)]


def assert_queued_calls_equal_synchronised_ones(make, one_shot, rows=lambda k: 1 + (5 * k) % 7):
    xs, queued, counts_q, state_q = alternate_one_shot_and_push(make, one_shot, rows, False)
    _, single, counts_s, state_s = alternate_one_shot_and_push(make, one_shot, rows, True)
    assert [x.size(0) for x in xs[::2]] == [1, 4, 7, 3, 6]
    assert counts_q == counts_s and state_q == state_s and state_q[0][0] == 5 * 500 and all(sum(c) > 0 for c in counts_q)
    for k, (q, s) in enumerate(zip(queued, single)):
        assert q.dtype == torch.int16 and q.shape == s.shape and torch.equal(q, s), f"call {k}"
    return xs, queued


def within_bar_i16(p, got, x, what):
    """an int16 output row: the rounding adds half a unit to the bar, the saturation nothing (a clamp never widens a distance)"""
    want, mag = RR.resample(p, x)
    err = np.abs(got.astype(np.float64) - np.clip(want, -32768, 32767))
    bar = RR.bar(p, mag) + 0.5
    print(f"{what}: worst error {float((err / bar).max()):.3f} of the bar")
    assert got.shape == want.shape and (err <= bar).all(), what


def test_one_shot_calls_and_pushes_share_one_ring():
    """one-shot calls and pushes of one handle, queued back to back through the one ring of row tables, equal the same calls made
    one at a time: outputs bit for bit, counts, and the streams' state"""
    lib = _capi.load()

    def one_shot(rs, x):
        B, n = int(x.size(0)), int(x.size(1))
        m = int(lib.wekws_hip_resample_num_samples(44100, 16000, n))
        out = torch.empty((B, m), dtype=torch.int16, device=DEV)
        _capi.check(lib.wekws_hip_resample_compute_i16(rs._ptr, x.data_ptr(), B, n, None, out.data_ptr(), m,
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "compute_i16")
        return out

    xs, queued = assert_queued_calls_equal_synchronised_ones(lambda: StreamingResampler(3, 44100, max_chunk=600), one_shot)
    within_bar_i16(plan(44100, 16000), queued[8][5].cpu().numpy(), xs[8][5].cpu().numpy(), "queued call 8 row 5")


def test_equal_rates_copy():
    rs = Resample(16000, 16000)
    x = torch.randint(-32768, 32768, (3, 1000), dtype=torch.int16, device=DEV)
    y, counts = rs(x, lengths=[1000, 0, 513])
    assert counts == [1000, 0, 513]
    want = x.to(torch.float32)
    want[1] = 0
    want[2, 513:] = 0
    assert torch.equal(y, want)


def step_rows(p):
    """row 0 random at full scale, row 1 a full-scale square wave (the filter overshoots at every step), row 2 alternating"""
    rng = np.random.default_rng(7)
    n = 2 * -(-TILE * p.o // p.n) + 3
    x = np.zeros((3, n), dtype=np.int16)
    x[0] = rng.integers(-32768, 32768, n)
    x[1] = np.where((np.arange(n) // (40 * max(1, round(p.o / p.n)))) % 2 == 0, 32767, -32768)
    x[2] = np.where(np.arange(n) % 2 == 0, 32767, -32767)
    return x


@pytest.mark.parametrize("orig,new", RR.PAIRS)
def test_int16_output_is_rint_and_saturation_of_the_float_output(orig, new):
    p = plan(orig, new)
    x = step_rows(p)
    want64, _ = RR.resample(p, x[1])
    assert (want64 > 32767.5).any() and (want64 < -32768.5).any(), "the oracle must saturate, or the test does not count"
    xi = torch.from_numpy(x).to(DEV)
    yf = Resample(orig, new)(xi).cpu().numpy()
    yq = Resample(orig, new, out_dtype=torch.int16)(xi)
    assert yq.dtype == torch.int16
    yq = yq.cpu().numpy()
    assert np.array_equal(yq, RR.to_i16(yf))
    assert (yq[1] == 32767).any() and (yq[1] == -32768).any()
    yq_f = Resample(orig, new, out_dtype=torch.int16)(xi.to(torch.float32)).cpu().numpy()
    assert np.array_equal(yq_f, yq)


def test_taps_rounded_to_fp16_miss_the_bar():
    """negative control: the bar tells float32 taps from half-precision ones"""
    hooks = C.CDLL(HOOKS)
    hooks.wekws_hip_debug_resample_round_taps_f16.restype = C.c_int
    hooks.wekws_hip_debug_resample_round_taps_f16.argtypes = [C.c_void_p]
    for orig, new in RR.PAIRS:
        p = plan(orig, new)
        x, lens = one_shot_rows(p)
        rs = Resample(orig, new)
        torch.cuda.synchronize()
        assert hooks.wekws_hip_debug_resample_round_taps_f16(rs._ptr) == 0
        got = rs(torch.from_numpy(x[4:5]).to(DEV), lengths=[lens[4]])[0].cpu().numpy()[0, :p.num_samples(lens[4])]
        want, mag = RR.resample(p, x[4, :lens[4]])
        ratio = np.abs(got - want) / RR.bar(p, mag)
        miss = float((ratio > 1).mean())
        print(f"{orig}->{new}: fp16 taps miss the bar at {miss:.1%} of the outputs, by up to {ratio.max():.0f}x")
        assert miss > 0.5


# ------------------------------------------------------------------------------------------ streaming
NS, SIG = 5, 6000


def run_pushes(rs, sig, pushes, flush_last=True, want_plan=None):
    """pushes: per push a list of (stream, n).  Returns each stream's concatenated output (device) and the counts of every push."""
    pos = [0] * NS
    outs = [[] for _ in range(NS)]
    all_counts = []
    for k, push in enumerate(pushes):
        ids = [s for s, _ in push]
        chunks = []
        for s, n in push:
            chunks.append(sig[s, pos[s]:pos[s] + n])
            pos[s] += n
        flush = flush_last and k == len(pushes) - 1
        out, counts = rs.push(chunks, streams=ids, flush=flush)
        if want_plan is not None:
            for (s, n), c in zip(push, counts):
                N, emitted = want_plan[s]
                total, _ = rs_plan(rs).step(N, n, flush)
                assert c == total - emitted, (k, s, n, c, total - emitted)
                want_plan[s] = (N + n, total)
        for b, s in enumerate(ids):
            assert not out[b, counts[b]:].any()
            outs[s].append(out[b, :counts[b]])
        all_counts.append(counts)
    return [torch.cat(o) if o else torch.zeros(0, dtype=rs.out_dtype, device=DEV) for o in outs], all_counts


def rs_plan(rs):
    return plan(rs.orig_freq, rs.new_freq)


def schedules(rng):
    primes = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113]
    every = list(range(NS))
    yield "all at once", [[(s, SIG) for s in every]]
    yield "1-sample chunks first", [[(s, 1) for s in every] for _ in range(200)] + [[(s, SIG - 200) for s in every]]
    cuts, left, k = [], SIG, 0
    while left > 0:
        n = min(primes[k % len(primes)] * (1 + k // len(primes)) * 7 // 5, left)
        cuts.append(n)
        left -= n
        k += 1
    yield "primes", [[(s, n) for s in every] for n in cuts]
    yield "with empty chunks", [[(s, n) for s in every] for n in (0, 1500, 0, 0, 2999, 1, 0, 1500, 0)]
    # a different schedule per stream, pushed as permuted subsets; the flush comes in a last push of empty chunks
    left = [SIG] * NS
    pushes = []
    while any(left):
        live = [s for s in every if left[s]]
        pick = [s for s in live if rng.random() < 0.7] or live[:1]
        pick = [pick[i] for i in rng.permutation(len(pick))]
        push = []
        for s in pick:
            n = min(int(rng.choice([1, 17, 160, 441, 997, 1600])), left[s])
            left[s] -= n
            push.append((s, n))
        pushes.append(push)
    yield "per-stream schedules, permuted subsets", pushes + [[(s, 0) for s in reversed(every)]]


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("orig,new", RR.PAIRS)
def test_streams_equal_the_one_shot_kernel_bit_for_bit(orig, new, out_dtype):
    rng = np.random.default_rng(orig + 1)
    sig = rng.integers(-32768, 32768, (NS, SIG), dtype=np.int16)
    want = Resample(orig, new, out_dtype=out_dtype)(torch.from_numpy(sig).to(DEV))
    rs = StreamingResampler(NS, orig, new, max_chunk=SIG, out_dtype=out_dtype)
    for name, pushes in schedules(rng):
        rs.reset()
        state = {s: (0, 0) for s in range(NS)}
        got, _ = run_pushes(rs, sig, pushes, want_plan=state)
        for s in range(NS):
            assert got[s].dtype == out_dtype and torch.equal(got[s], want[s]), (name, s)
            assert rs.counts(s) == (SIG, want.size(1), 0, 1)


@pytest.mark.parametrize("orig,new", RR.PAIRS)
def test_reset_refusals_and_queued_pushes(orig, new):
    rng = np.random.default_rng(orig + 2)
    sig = rng.integers(-32768, 32768, (NS, SIG), dtype=np.int16)
    one = Resample(orig, new, out_dtype=torch.int16)
    want = one(torch.from_numpy(sig).to(DEV))
    every = list(range(NS))
    cuts = [500] * 12
    pushes = [[(s, n) for s in every] for n in cuts]
    # ---- twelve pushes queued back to back (the table ring holds four) == synchronised ones
    rs = StreamingResampler(NS, orig, new, max_chunk=2000)
    dsig = torch.from_numpy(sig).to(DEV)
    torch.cuda.synchronize()
    queued = [rs.push(dsig[:, 500 * k:500 * (k + 1)], flush=(k == 11)) for k in range(12)]
    torch.cuda.synchronize()
    got = torch.cat([o[:, :max(c)] for o, c in queued], dim=1)
    assert all(len(set(c)) == 1 for _, c in queued)
    rs.reset()
    synced = []
    for k in range(12):
        synced.append(rs.push(dsig[:, 500 * k:500 * (k + 1)], flush=(k == 11)))
        torch.cuda.synchronize()
    assert [c for _, c in queued] == [c for _, c in synced]
    assert torch.equal(got, torch.cat([o[:, :max(c)] for o, c in synced], dim=1)) and torch.equal(got, want)
    # ---- reset of one stream mid-way; refused pushes in between change nothing
    rs.reset()
    first, _ = run_pushes(rs, sig, pushes[:5], flush_last=False)
    rs.reset([2])
    assert rs.counts(2) == (0, 0, 0, 0) and rs.counts(1)[0] == 2500
    chunk = torch.zeros((2, 100), dtype=torch.int16, device=DEV)
    for kw, msg in ((dict(streams=[0, NS]), "outside"), (dict(streams=[1, 1]), "twice"), (dict(streams=[0, 1], samples=[5, 101]), "samples"),
                    (dict(streams=[0, 1], capacity=3), "mcap")):
        with pytest.raises(_capi.HipLibraryError, match=msg):
            rs.push(chunk, **kw)
    with pytest.raises(_capi.HipLibraryError, match="max_chunk"):
        rs.push(torch.zeros((1, 2001), dtype=torch.int16, device=DEV), streams=[3])
    rest = []
    pos = 2500
    for k in range(5, 12):
        ids = [4, 2, 0, 3, 1]
        chunks = [sig[s, (pos - 2500 if s == 2 else pos):(pos - 2500 if s == 2 else pos) + 500] for s in ids]
        out, counts = rs.push(chunks, streams=ids, flush=(k == 11))
        rest.append({s: out[b, :counts[b]] for b, s in enumerate(ids)})
        pos += 500
    for s in every:
        tail = torch.cat([r[s] for r in rest])
        if s == 2:       # started over: the one-shot result of what it was given after the reset
            again = one(torch.from_numpy(sig[2:3, :3500].copy()).to(DEV))[0]
            assert torch.equal(tail, again)
        else:
            assert torch.equal(torch.cat([first[s], tail]), want[s]), s
    # ---- a push after the flush is refused until the stream is reset
    with pytest.raises(_capi.HipLibraryError, match="flushed"):
        rs.push(chunk[:1], streams=[0])
    assert rs.counts(0) == (SIG, want.size(1), 0, 1)
    rs.reset([0])
    out, counts = rs.push(chunk[:1], streams=[0])
    assert counts[0] == rs_plan(rs).step(0, 100, False)[0] and not out.any()


# ------------------------------------------------------------------------------------------ non-finite
def test_non_finite_samples_follow_the_full_window():
    orig, new = 44100, 16000
    p = plan(orig, new)
    rng = np.random.default_rng(11)
    L = 3 * 706 + 50
    clean = rng.uniform(-3e4, 3e4, (3, L)).astype(np.float32)
    rs = Resample(orig, new)
    base = rs(torch.from_numpy(clean).to(DEV)).cpu().numpy()
    # output q = 3 n + 5 (block j = 3, phase 5): a position under one of its live taps, and one inside its K-tap window under a
    # tap the clamp zeroes
    j, i = 3, 5
    live_pos = j * p.o + int(p.first[i]) + 4 - p.width
    dead_pos = j * p.o + int(p.last[i]) + 40 - p.width
    assert p.live[i, p.first[i] + 4] and not p.live[i, p.last[i] + 40] and p.taps[i, p.last[i] + 40] == 0 and p.last[i] + 40 < p.K
    for val in (np.nan, np.inf, -np.inf):
        for pos in (live_pos, dead_pos):
            x = clean.copy()
            x[1, pos] = val
            got = rs(torch.from_numpy(x).to(DEV)).cpu().numpy()
            assert np.array_equal(got[0].view(np.int32), base[0].view(np.int32)) and np.array_equal(got[2].view(np.int32), base[2].view(np.int32))
            want_cls = RR.classes(p, x[1])
            assert np.array_equal(RR.classify(got[1]), want_cls), (val, pos)
            assert want_cls[j * p.n + i] != 0 and (want_cls != 0).sum() >= p.n
            want, mag = RR.resample(p, x[1])
            fin = want_cls == 0
            assert fin.sum() > 100 and (np.abs(got[1][fin] - want[fin]) <= RR.bar(p, mag)[fin]).all(), (val, pos)


# ------------------------------------------------------------------------------------------ scale
def test_4096_streams_in_one_push():
    orig, new = 48000, 16000
    p = plan(orig, new)
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randint(-32768, 32768, (4096, 4800), dtype=torch.int16, generator=g)
    xd = x.to(DEV)
    for dt in (torch.float32, torch.int16):
        rs = StreamingResampler(4096, orig, new, max_chunk=4800, out_dtype=dt)
        out, counts = rs.push(xd, flush=True)
        want = Resample(orig, new, out_dtype=dt)(xd)
        assert counts == [1600] * 4096 and torch.equal(out, want)
    got = Resample(orig, new)(xd)
    rows = np.random.default_rng(5).choice(4096, 64, replace=False)
    gh = got[torch.from_numpy(rows).to(DEV)].cpu().numpy()
    xs = x.numpy()
    worst = max(within_bar(p, gh[k], xs[r], f"row {r}") for k, r in enumerate(rows))
    assert worst <= 1.0
