"""CPU: the per-stream plan of the streaming front end (wekws_amd/csrc/stream_frontend.h through
wekws_hip_stream_frontend_plan) against the index-space restatement (tests/stream_frontend_ref.py), and the restatement
against the live reference's accept_wave (tests/golden/stream_frontend_golden.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import splice_oracle
from tests import stream_frontend_ref as sref
from wekws_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "stream_frontend_golden.npz"))


def make_cfg(L=400, S=160, left=0, right=0, skip=1, bins=40, window=0, max_streams=4, max_chunk=4800, rate=16000):
    cfg = _capi.StreamFrontendCfg()
    cfg.fbank.num_bins, cfg.fbank.sample_rate, cfg.fbank.frame_length, cfg.fbank.frame_shift = bins, rate, L, S
    cfg.fbank.window = window
    cfg.left, cfg.right, cfg.skip, cfg.max_streams, cfg.max_chunk, cfg.device = left, right, skip, max_streams, max_chunk, 0
    return cfg


def plan(cfg, counts, n):
    """(rc, dict) of wekws_hip_stream_frontend_plan."""
    out = (C.c_int32 * 10)()
    rc = _capi.load().wekws_hip_stream_frontend_plan(C.byref(cfg), (C.c_int32 * 3)(*counts), int(n), out)
    keys = ("status", "held", "nf", "rem_out", "pad_first", "fr_in", "rows_ctx", "rows_out", "fr_out", "off_out")
    return rc, dict(zip(keys, (int(v) for v in out)))


def offsets(L):
    return np.array([0, 1, L // 2, L - 1])


def test_golden_is_small_and_integer(golden):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "stream_frontend_golden.npz")) < 256 * 1024
    names = [str(n) for n in golden["names"]]
    assert len(names) >= 20
    for n in names:
        for key in ("cfg", "n", "kind", "counts", "rows"):
            assert golden[f"{key}/{n}"].dtype == np.int32
    cfgs = {tuple(int(v) for v in golden[f"cfg/{n}"][2:]) for n in names}
    assert {(0, 0, 1), (0, 0, 3), (2, 2, 3), (1, 1, 2), (2, 2, 1), (3, 3, 2)} <= cfgs
    kinds = np.concatenate([golden[f"kind/{n}"] for n in names])
    sizes = np.concatenate([golden[f"n/{n}"] for n in names])
    assert (kinds == -1).any() and (kinds == -2).any() and (kinds == 0).any()          # held, assertion, empty
    assert (sizes == 0).any() and (sizes == 1).any() and (sizes % 2 == 1).any()
    assert any(int(golden[f"cfg/{n}"][1]) != 160 for n in names)
    # a push of fewer than 2 r frames: afterwards fewer than left + right frames are remembered
    assert any(((golden[f"counts/{n}"][:, 1] >= 0) & (golden[f"counts/{n}"][:, 1] < 2 * golden[f"cfg/{n}"][3])).any()
               for n in names if golden[f"cfg/{n}"][3] > 0)


def test_restatement_reproduces_the_reference(golden):
    """Every returned row, hold, assertion and count of the live reference, for every golden schedule."""
    for name in (str(n) for n in golden["names"]):
        L, S, left, right, skip = (int(v) for v in golden[f"cfg/{name}"])
        sizes, kinds, counts, rows = (golden[f"{k}/{name}"] for k in ("n", "kind", "counts", "rows"))
        got = sref.run_schedule(L, S, left, right, skip, sizes)
        assert len(got) == len(kinds), name
        at = 0
        for i, (res, cnt) in enumerate(got):
            if kinds[i] == -2:
                assert sref.is_marker(res, sref.ASSERT), (name, i)
                continue
            assert tuple(int(v) for v in counts[i]) == cnt, (name, i, counts[i], cnt)
            if kinds[i] == -1:
                assert sref.is_marker(res, sref.HELD), (name, i)
                continue
            assert not isinstance(res, str) and res.shape[0] == kinds[i], (name, i)
            want = rows[at:at + kinds[i]]
            at += int(kinds[i])
            samples = (res[:, :, None] * S + offsets(L)[None, None, :]).reshape(res.shape[0], res.shape[1] * 4)
            assert np.array_equal(samples, want), (name, i)
        assert at == rows.shape[0], name


def check_stream_against_plan(cfg, ref, sizes, what):
    """Feed `sizes` to the restatement and to the C plan, carrying the plan's own counts: equal at every push."""
    counts = (0, -1, 0)
    for i, n in enumerate(sizes):
        before = ref.counts()
        assert before == counts, (what, i)
        res = ref.push(int(n))
        rc, p = plan(cfg, counts, n)
        assert rc == 0, (what, i, _capi.last_error())
        if sref.is_marker(res, sref.ASSERT):
            assert p["status"] == EINVAL, (what, i, p)
            break
        assert p["status"] == 0, (what, i, p)
        assert p["held"] == int(sref.is_marker(res, sref.HELD)), (what, i, p)
        rows = 0 if p["held"] else res.shape[0]
        assert p["rows_out"] == rows, (what, i, p, rows)
        counts = (p["rem_out"], p["fr_out"], p["off_out"])
        assert counts == ref.counts(), (what, i, p, ref.counts())
        L, r = ref.L, ref.r
        assert 0 <= p["rem_out"] < max(L, L * r), (what, i, p)
        assert p["rem_out"] == before[0] + n - p["nf"] * ref.S
        if not p["held"] and ref.ctx:
            assert p["pad_first"] == int(before[1] < 0) and p["fr_in"] == max(before[1], 0), (what, i, p)


def test_plan_equals_restatement_on_golden_schedules(golden):
    for name in (str(n) for n in golden["names"]):
        L, S, left, right, skip = (int(v) for v in golden[f"cfg/{name}"])
        cfg = make_cfg(L, S, left, right, skip)
        check_stream_against_plan(cfg, sref.StreamRef(L, S, left, right, skip), golden[f"n/{name}"], name)


def test_plan_equals_restatement_on_random_streams():
    """2,400 seeded streams of random pushes (0 / 1 / odd sizes, several frame shifts and contexts)."""
    rng = np.random.default_rng(7)
    configs = [(400, 160, 0, 0, 1), (400, 160, 0, 0, 3), (400, 160, 2, 2, 3), (400, 160, 1, 1, 2), (400, 160, 2, 2, 1),
               (400, 160, 3, 3, 2), (200, 80, 1, 1, 1), (320, 80, 2, 2, 3), (400, 100, 0, 0, 2), (512, 512, 1, 1, 3),
               (401, 161, 2, 2, 2), (480, 33, 0, 0, 4)]
    special = np.array([0, 1, 2, 3, 159, 160, 161, 399, 400, 401, 4800])
    streams = 0
    for L, S, left, right, skip in configs:
        cfg = make_cfg(L, S, left, right, skip)
        for _ in range(200):
            k = int(rng.integers(3, 25))
            sizes = np.where(rng.random(k) < 0.4, rng.choice(special, k), rng.integers(0, 5001, k))
            check_stream_against_plan(cfg, sref.StreamRef(L, S, left, right, skip), sizes, (L, S, left, right, skip))
            streams += 1
    assert streams >= 2000


def test_frames_without_context_are_the_frames_of_the_samples_so_far():
    rng = np.random.default_rng(11)
    for L, S, skip in ((400, 160, 1), (200, 80, 1), (400, 100, 1)):
        cfg = make_cfg(L, S, 0, 0, skip)
        for _ in range(50):
            counts, total, frames = (0, -1, 0), 0, 0
            for n in rng.integers(0, 3000, size=12):
                rc, p = plan(cfg, counts, n)
                assert rc == 0 and p["status"] == 0 and p["held"] == 0
                counts = (p["rem_out"], p["fr_out"], p["off_out"])
                total += int(n)
                frames += p["rows_out"]
                assert frames == (0 if total < L else 1 + (total - L) // S)


@pytest.mark.parametrize("left,right,skip", [(2, 2, 3), (1, 1, 2), (2, 2, 1), (3, 3, 2), (0, 0, 3)])
def test_stream_rows_equal_the_one_shot_splice(left, right, skip):
    """With chunks of at least 2 r frames the concatenated rows are the one-shot splice_skip of the whole index sequence
    (all of it: left == right makes the stream's row count sum(nf) - r, the one-shot's T - right)."""
    rng = np.random.default_rng(3)
    L, S = 400, 160
    for _ in range(20):
        ref = sref.StreamRef(L, S, left, right, skip)
        rows, total = [], 0
        for n in rng.integers(S * (2 * right + 3), 5000, size=10):
            res = ref.push(int(n))
            total += int(n)
            if not isinstance(res, str):
                rows.append(res)
        got = np.concatenate(rows)
        nf = 1 + (total - L) // S
        whole = np.arange(nf, dtype=np.float32).reshape(1, nf, 1)
        want = splice_oracle.splice_skip(whole, left, right, skip)[0].astype(np.int64)
        assert np.array_equal(got, want)


def test_refused_configurations():
    lib = _capi.load()
    out = (C.c_int32 * 10)()
    zero = (C.c_int32 * 3)(0, -1, 0)
    bad = [dict(left=1, right=2), dict(left=2, right=1), dict(left=0, right=2), dict(left=-1, right=-1), dict(skip=0),
           dict(S=0), dict(S=401), dict(L=0), dict(bins=0), dict(bins=129), dict(window=2), dict(L=513, S=160)]
    for kw in bad:
        cfg = make_cfg(**kw)
        assert lib.wekws_hip_stream_frontend_plan(C.byref(cfg), zero, 100, out) == EINVAL, kw
        assert _capi.last_error() != ""
        h = C.c_void_p()
        assert lib.wekws_hip_stream_frontend_create(C.byref(cfg), C.byref(h)) == EINVAL and not h, kw
    for kw in (dict(max_streams=0), dict(max_chunk=0)):
        h = C.c_void_p()
        cfg = make_cfg(**kw)
        assert lib.wekws_hip_stream_frontend_create(C.byref(cfg), C.byref(h)) == EINVAL and not h, kw
    assert "left" in (lib.wekws_hip_stream_frontend_plan(C.byref(make_cfg(left=1, right=2)), zero, 1, out), _capi.last_error())[1]
    # counts no stream can have
    cfg = make_cfg(left=2, right=2, skip=3)
    for counts, n in (((-1, -1, 0), 1), ((800, -1, 0), 1), ((0, 5, 0), 1), ((0, -2, 0), 1), ((0, -1, 3), 1), ((0, -1, 0), -1)):
        assert lib.wekws_hip_stream_frontend_plan(C.byref(cfg), (C.c_int32 * 3)(*counts), n, out) == EINVAL, (counts, n)


def test_struct_layout():
    assert C.sizeof(_capi.StreamFrontendCfg) == (8 + 8) * 4
