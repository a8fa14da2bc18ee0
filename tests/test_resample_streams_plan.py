"""CPU: the stream planner of both resampler handles (wekws_amd/csrc/resample_streams.h), without a device.

wekws_hip_debug_resample_streams_script drives the planner through a schedule of pushes, resets and set_rates.  After every accepted
push the row table -- as it is uploaded, in slot order -- and the counts of every stream are held to a restatement in Python integers,
built from tests/resample_ref.py's Plan.step and the field definitions in ResampleRow's comments (resample.hip.h).  Between the
accepted calls come refused ones: each names its refusal and its row and changes no stream.  The same schedule on a one-member bank
gives the same rows whether it is planned as a bank or as the single-rate handle: one member IS the single-rate handle."""
import ctypes as C
import os

import numpy as np

from tests import resample_ref as RR
from wekws_amd import _capi

HOOKS = os.path.join(os.path.dirname(_capi.lib_path()), "libwekws_hip_hooks.so")
BANK = (8000, 44100, 48000)
NEW, NS, MAX_CHUNK = 16000, 5, 700
FIELDS = ("i0", "base_rel", "cnt", "h", "hi_valid", "hist_old", "hist_new", "keep_from", "keep_cnt", "member", "row", "wire")
OK, ID, TWICE, ROWS, FLUSHED, INTERNAL, CAP = range(7)          # ResampleStreamsRefusal
ROWS_LENGTH = 4                                                 # ResampleBankRowRefusal


class Streams:
    """The restatement: what a handle's streams are, in Python integers."""

    def __init__(self, rates):
        self.plans = [RR.Plan(r, NEW) for r in rates]
        self.hist_cap = max((int((p.last - p.first + 1).max()) + 1) & ~1 for p in self.plans)
        self.received, self.emitted, self.origin = [0] * NS, [0] * NS, [0] * NS
        self.par, self.flushed, self.member = [0] * NS, [0] * NS, [0] * NS

    def counts(self):
        return [[self.received[i], self.emitted[i], self.received[i] - self.origin[i], self.flushed[i]] for i in range(NS)]

    def need_cap(self, ids, nsamp, flush):
        return max(self.plans[self.member[i]].step(self.received[i], n, flush)[0] - self.emitted[i] for i, n in zip(ids, nsamp))

    def push(self, ids, nsamp, flush):
        """the rows in slot order (sorted by member, stable); the streams move"""
        rows = []
        for b, (i, n) in enumerate(zip(ids, nsamp)):
            p = self.plans[self.member[i]]
            total, keep = p.step(self.received[i], n, flush)
            q0, s0 = self.emitted[i], self.origin[i]
            j0, i0 = divmod(q0, p.n)
            h = self.received[i] - s0
            rows.append(dict(i0=i0, base_rel=j0 * p.o - p.width - s0, cnt=total - q0, h=h, hi_valid=h + n,
                             hist_old=(2 * i + self.par[i]) * self.hist_cap, hist_new=(2 * i + (self.par[i] ^ 1)) * self.hist_cap,
                             keep_from=keep - s0, keep_cnt=self.received[i] + n - keep, member=self.member[i], row=b, wire=0))
            assert 0 <= rows[-1]["keep_cnt"] <= self.hist_cap and keep >= s0
            self.received[i] += n
            self.emitted[i], self.origin[i] = total, keep
            self.par[i] ^= 1
            self.flushed[i] |= int(bool(flush))
        order = np.argsort([r["member"] for r in rows], kind="stable")
        return [[rows[k][f] for f in FIELDS] for k in order]

    def reset(self, ids, member=None):
        for i in ids:
            if member is not None:
                self.member[i] = member
            self.received[i] = self.emitted[i] = self.origin[i] = self.flushed[i] = 0


def schedule(ref, members):
    """The calls, each (script ints, expected refusal, expected row, expected rows or None); ref moves along.  members: the member
    each stream is given (one per stream), and the one stream 3 changes to mid-way."""
    rng = np.random.default_rng(20241020)
    calls = []

    def push(ids, nsamp, flush=0, width=MAX_CHUNK, mcap=None, refusal=OK, row=-1):
        ids, nsamp = [int(v) for v in ids], [int(v) for v in nsamp]
        if mcap is None:
            mcap = 4000                                         # (more than any row of 700 samples yields: 8000 -> 16000 doubles)
        script = [0, 0, len(ids), width, flush, mcap] + ids + nsamp
        calls.append((script, refusal, row, ref.push(ids, nsamp, flush) if refusal == OK else None))

    def reset(ids, member=None):
        calls.append(([1, len(ids)] + ids if member is None else [2, member, len(ids)] + ids, 0, -1, None))
        ref.reset(ids, member)

    for i, m in enumerate(members[:NS]):
        reset([i], m)
    for k in range(12):
        last = k == 11
        ids = rng.permutation(NS)[:NS if last else int(rng.integers(1, NS + 1))]
        ids = [int(i) for i in ids if not ref.flushed[i]]
        nsamp = rng.integers(0, MAX_CHUNK + 1, len(ids))
        if k in (3, 9):
            nsamp[0] = 0                                        # a row that brings nothing
        if k == 5:
            nsamp[:] = MAX_CHUNK
        push(ids, nsamp, flush=int(last))
        # ---- the refused calls, one after each of the first pushes
        if k == 0:
            push([1, NS, 0], [5, 5, 5], refusal=ID, row=1)
            push([1, -1], [5, 5], refusal=ID, row=1)
        elif k == 1:
            push([2, 0, 3, 0], [5, 5, 5, 5], refusal=TWICE, row=3)
        elif k == 2:
            push([4, 2], [10, 601], width=600, refusal=ROWS, row=1)              # longer than the row (nmax)
        elif k == 3:
            push([0, 1, 3], [700, 700, 701], width=800, refusal=ROWS, row=2)     # longer than max_chunk
        elif k == 4:
            ids, nsamp = [3, 1, 4, 0], [700, 300, 0, 650]
            need = ref.need_cap(ids, nsamp, 0)
            assert need > 1
            push(ids, nsamp, mcap=need - 1, refusal=CAP, row=-1)
            push(ids, nsamp, mcap=need)                                          # ... and with exactly need_cap it is taken
        elif k == 5:
            reset([2])
            reset([3], members[NS])
        elif k == 6:
            push([4], [123], flush=1)                                            # stream 4 ends early ...
            push([0, 4], [5, 5], refusal=FLUSHED, row=1)
        elif k == 7:
            push([4, 0], [0, 5], flush=1, refusal=FLUSHED, row=0)
            reset([4])                                                           # ... and starts over
    assert all(ref.flushed)
    return calls


def run(rates, single, calls):
    lib = C.CDLL(HOOKS)
    fn = lib.wekws_hip_debug_resample_streams_script
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                   C.c_void_p, C.c_void_p, C.c_void_p]
    r = np.asarray(rates, dtype=np.int32)
    script = np.asarray([v for c in calls for v in c[0]], dtype=np.int32)
    n = len(calls)
    outcome = np.full((n, 4), -7, dtype=np.int64)
    rows = np.full((n, NS, 12), -7, dtype=np.int32)
    counts = np.full((n, NS, 4), -7, dtype=np.int64)
    assert fn(r.ctypes.data, None, r.size, NEW, 6, 0.99, single, NS, MAX_CHUNK, script.ctypes.data, script.size, n, outcome.ctypes.data,
              rows.ctypes.data, counts.ctypes.data) == n
    return outcome, rows, counts


def check(rates, single, members):
    ref = Streams(rates)
    live = Streams(rates)                                       # follows the accepted calls: the counts after every call
    calls = schedule(ref, members)
    outcome, rows, counts = run(rates, single, calls)
    accepted = refused = 0
    for k, (script, refusal, row, want) in enumerate(calls):
        before = live.counts()
        assert (int(outcome[k, 0]), int(outcome[k, 1])) == (refusal, row), (k, script, outcome[k])
        if script[0] != 0:
            live.reset(script[2:] if script[0] == 1 else script[3:], None if script[0] == 1 else script[1])
        elif refusal == OK:
            B = script[2]
            assert live.push(script[6:6 + B], script[6 + B:6 + 2 * B], script[4]) == want
            assert rows[k, :B].tolist() == want, (k, script)
            assert (rows[k, B:] == -7).all(), "nothing is written past the table"
            accepted += 1
        else:
            assert counts[k].tolist() == before, ("a refused call moved a stream", k, script)
            if refusal == ROWS:
                assert outcome[k, 2] == ROWS_LENGTH
            refused += 1
        assert counts[k].tolist() == live.counts(), (k, script)
    assert accepted >= 13 and refused == 8
    return outcome, rows, counts


def test_bank_schedule_equals_the_restatement():
    outcome, rows, counts = check(BANK, 0, [0, 1, 2, 0, 1, 2])
    # the schedule did what it is for: rows of every member, slot order that is not row order, a stream that kept history
    taken = outcome[:, 0] == OK
    assert set(rows[taken][:, :, 9].ravel().tolist()) >= {0, 1, 2}
    assert any((np.diff(t[t[:, 10] >= 0, 10]) < 0).any() for t in rows[taken])
    assert (rows[taken][:, :, 3] > 0).any() and counts[-1, :, 3].all()


def test_one_member_is_the_single_rate_handle():
    members = [0] * (NS + 1)
    single = check((44100,), 1, members)
    bank = check((44100,), 0, members)
    outcome, rows, _ = single
    taken = outcome[:, 0] == OK
    # (the most outputs of a row "as far as planned" is the one thing that may differ, in a refused call: row by row gets further)
    assert np.array_equal(single[0][:, :3], bank[0][:, :3]) and np.array_equal(single[0][taken, 3], bank[0][taken, 3])
    assert np.array_equal(single[1], bank[1]) and np.array_equal(single[2], bank[2])
    B = rows[taken][:, :, 10] >= 0
    assert (rows[taken][:, :, 9][B] == 0).all() and (rows[taken][:, :, 11][B] == 0).all()
    # one member: slot order is row order
    assert all(t[t[:, 10] >= 0, 10].tolist() == list(range(int((t[:, 10] >= 0).sum()))) for t in rows[taken])


def test_a_call_with_two_faults_names_the_one_its_handle_always_named():
    """Row 0 names a flushed stream, row 1 a stream outside the range.  The bank looks at every row's id before any stream's state; the
    single-rate handle goes row by row."""
    calls = [([0, 0, 1, MAX_CHUNK, 1, 4000, 0, 10], OK, -1, None), ([0, 0, 2, MAX_CHUNK, 0, 4000, 0, NS, 10, 10], None, None, None)]
    assert run((44100,), 0, calls)[0][1, :2].tolist() == [ID, 1]
    assert run((44100,), 1, calls)[0][1, :2].tolist() == [FLUSHED, 0]


def test_malformed_scripts_are_refused():
    lib = C.CDLL(HOOKS)
    fn = lib.wekws_hip_debug_resample_streams_script
    fn.restype = C.c_int
    r = np.asarray(BANK, dtype=np.int32)
    out = np.zeros(4096, dtype=np.int64)
    for script, single in (([7], 0), ([0, 0, 2, 700, 0, 10, 1], 0), ([2, 3, 1, 0], 0), ([1, 1, 0], 1)):
        s = np.asarray(script, dtype=np.int32)
        assert fn(C.c_void_p(r.ctypes.data), None, 3, NEW, 6, C.c_double(0.99), single, NS, MAX_CHUNK, C.c_void_p(s.ctypes.data), s.size, 4,
                  C.c_void_p(out.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(out.ctypes.data)) < 0
