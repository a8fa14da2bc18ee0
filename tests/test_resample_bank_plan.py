"""CPU: the host plan of the rate bank (wekws_amd/csrc/resample_bank_plan.h) and the creation-time refusals of
wekws_hip_resample_bank_create, without a device.

The bank's sizes are held to the maxima over its members' single-rate plans (wekws_hip_debug_resample_plan); the tile order of a
launch -- which (row, tile) every workgroup walks -- is held to its four properties over seeded cases."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import resample_ref as RR
from wekws_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = os.path.join(os.path.dirname(_capi.lib_path()), "libwekws_hip_hooks.so")
BANK = (48000, 8000, 44100, 24000, 16000)
NAMES = ["create", "destroy", "compute", "compute_i16", "set_rate", "rate_of", "push", "max_out", "reset", "counts"]
DEBUG = ["plan", "set_grid", "round_taps_f16"]


@pytest.fixture(scope="module")
def hooks():
    lib = C.CDLL(HOOKS)
    lib.wekws_hip_debug_resample_plan.restype = C.c_int
    lib.wekws_hip_debug_resample_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int64,
                                                  C.c_void_p, C.c_void_p, C.c_int64]
    lib.wekws_hip_debug_resample_step.restype = C.c_int
    lib.wekws_hip_debug_resample_step.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    lib.wekws_hip_debug_resample_bank_plan.restype = C.c_int
    lib.wekws_hip_debug_resample_bank_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]
    return lib


def bank_plan(hooks, rates, nmax=0, flush=0, new=16000):
    r = np.asarray(rates, dtype=np.int32)
    dims, bad = np.zeros(4, dtype=np.int64), C.c_int(-2)
    rc = hooks.wekws_hip_debug_resample_bank_plan(r.ctypes.data, r.size, new, 6, 0.99, nmax, flush, dims.ctypes.data, C.byref(bad),
                                                  None, 0, 0, 0, None, None, None)
    return rc, [int(v) for v in dims], bad.value


def tile_order(hooks, rates, member_of_row, tiles_per_row, grid):
    r = np.asarray(rates, dtype=np.int32)
    mem = np.ascontiguousarray(member_of_row, dtype=np.int32)
    total = mem.size * tiles_per_row
    dims = np.zeros(4, dtype=np.int64)
    rows, tiles = np.full(total + 1, -7, dtype=np.int32), np.full(total + 1, -7, dtype=np.int32)
    spans = np.full(grid + 2, -7, dtype=np.int64)
    rc = hooks.wekws_hip_debug_resample_bank_plan(r.ctypes.data, r.size, 16000, 6, 0.99, 0, 0, dims.ctypes.data, None, mem.ctypes.data,
                                                  mem.size, tiles_per_row, grid, rows.ctypes.data, tiles.ctypes.data, spans.ctypes.data)
    assert rc == 0
    assert rows[total] == -7 and tiles[total] == -7 and spans[grid + 1] == -7, "nothing is written past the list"
    return rows[:total], tiles[:total], spans[:grid + 1]


def make_cfg(orig, new=16000, max_streams=0, max_chunk=0, lpw=6, rolloff=0.99, out=0):
    c = _capi.ResampleCfg()
    c.orig_freq, c.new_freq, c.lowpass_filter_width, c.out_dtype, c.rolloff = orig, new, lpw, out, rolloff
    c.max_streams, c.max_chunk, c.device = max_streams, max_chunk, 0
    return c


def create(lib, rates, cfg=None):
    h = C.c_void_p()
    arr = (C.c_int32 * max(len(rates), 1))(*rates)
    rc = lib.wekws_hip_resample_bank_create(C.byref(cfg if cfg is not None else make_cfg(rates[0] if rates else 48000)), arr,
                                            len(rates), C.byref(h))
    return rc, h


def test_symbols_and_signatures():
    lib = _capi.load()
    src = open(os.path.join(ROOT, "include", "wekws_hip.h")).read()
    for n in NAMES:
        name = "wekws_hip_resample_bank_" + n
        assert hasattr(lib, name) and name in _capi.SIGNATURES and name + "(" in src, name
    assert "#define WEKWS_HIP_ABI_VERSION 2" in src and "#define WEKWS_HIP_RESAMPLE_BANK_MAX 16" in src
    # the debug entry points are the hooks library's alone
    hooks = C.CDLL(HOOKS)
    for n in DEBUG:
        assert hasattr(hooks, "wekws_hip_debug_resample_bank_" + n) and not hasattr(lib, "wekws_hip_debug_resample_bank_" + n)
    assert "wekws_hip_debug" not in src


def test_create_time_refusals():
    import torch
    lib = _capi.load()
    for rates, what in (([], "1..16"), (list(range(8000, 8000 + 17)), "1..16"), ([48000, 8000, 48000], "repeats"),
                        ([48000, 0], "positive"), ([48000, -8000], "positive")):
        rc, h = create(lib, rates)
        assert rc == -1 and not h and what in _capi.last_error(), (rates, rc, _capi.last_error())
    rc, h = create(lib, [48000, 8000], make_cfg(8000))
    assert rc == -1 and not h and "member 0" in _capi.last_error()
    for mc in (0, -5):
        rc, h = create(lib, [48000, 8000], make_cfg(48000, max_streams=4, max_chunk=mc))
        assert rc == -1 and not h and "max_chunk" in _capi.last_error()
    rc, h = create(lib, [48000, 44101, 8000])
    assert rc == -4 and not h                                                           # EUNSUPPORTED
    assert "44101" in _capi.last_error() and "member 1" in _capi.last_error() and "LDS" in _capi.last_error()
    assert lib.wekws_hip_resample_bank_create(None, None, 0, C.byref(h)) == -1
    if not torch.cuda.is_available():
        # a supported bank gets as far as the device
        for rates, ms in ((list(BANK), 8), ([16000], 0), ([8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000, 16000], 4)):
            rc, h = create(lib, rates, make_cfg(rates[0], max_streams=ms, max_chunk=4800 if ms else 0))
            assert rc == -3 and not h, (rates, rc, _capi.last_error())
    assert lib.wekws_hip_resample_bank_push(None, None, 1, 1, None, None, 0, None, 0, None, None) == -1
    assert lib.wekws_hip_resample_bank_compute(None, None, 1, 1, None, None, None, 0, None) == -1
    assert lib.wekws_hip_resample_bank_set_rate(None, None, 0, 0) == -1 and lib.wekws_hip_resample_bank_rate_of(None, 0) == -1
    assert lib.wekws_hip_resample_bank_max_out(None, 5, 0) == 0


def test_plan_refusals_name_the_member(hooks):
    assert bank_plan(hooks, [])[0] == -1 and bank_plan(hooks, list(range(1, 18)))[0] == -1
    assert bank_plan(hooks, [48000, 8000, 8000])[::2] == (-1, 2)
    assert bank_plan(hooks, [48000, 8000, -1, 16000])[::2] == (-1, 2)
    assert bank_plan(hooks, [48000, 8000, 24000, 44101])[::2] == (-4, 3)
    rc, dims, bad = bank_plan(hooks, [8000 * k for k in range(1, 17)])
    assert (rc, dims[3], bad) == (0, 16, -1)


def test_derived_sizes_are_the_members_maxima(hooks):
    members = []
    for r in BANK:
        dims = np.zeros(10, dtype=np.int64)
        assert hooks.wekws_hip_debug_resample_plan(r, 16000, 6, 0.99, dims.ctypes.data, None, 0, None, None, 0) == 0
        members.append(dims)
    for nmax, flush in ((0, 0), (1, 1), (480, 0), (4800, 1), (14400, 0), (14400, 1)):
        rc, dims, bad = bank_plan(hooks, BANK, nmax, flush)
        assert rc == 0 and bad == -1 and dims[3] == len(BANK)
        assert dims[0] == max(int(d[6]) for d in members) <= 64 * 1024
        assert dims[1] == max(int(d[8]) for d in members)
        outs = []
        for r in BANK:
            out = np.zeros(4, dtype=np.int64)
            assert hooks.wekws_hip_debug_resample_step(r, 16000, 6, 0.99, 0, nmax, flush, out.ctypes.data) == 0
            outs.append(int(out[3]))
        assert dims[2] == max(outs)
    # the maxima come from different members: the sizes are not one member's
    assert int(np.argmax([int(d[6]) for d in members])) == BANK.index(44100)
    rc, dims, _ = bank_plan(hooks, BANK, 4800, 0)
    assert dims[2] == RR.Plan(8000, 16000).num_samples(4800) + 2                       # the up-sampling member decides max_out
    # a one-member bank has that member's sizes
    for r, d in zip(BANK, members):
        rc, dims, _ = bank_plan(hooks, [r], 1000, 1)
        assert rc == 0 and dims[:2] == [int(d[6]), int(d[8])]


def test_tile_order_over_seeded_cases(hooks):
    rng = np.random.default_rng(2024)
    rates = [8000 * k for k in range(1, 17)]
    cases = changes_seen = 0
    for _ in range(300):
        num = int(rng.integers(1, 17))
        B = int(rng.integers(0, 40))
        tpr = int(rng.choice([1, 1, 2, 3, 5, 19]))
        total = B * tpr
        grid = int(rng.choice([1, 2, 3, max(total // 3, 1), max(total - 1, 1), max(total, 1), total + 1, total + 7, 2048]))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            mem = rng.integers(0, num, B)                            # any member anywhere
        elif kind == 1:
            mem = np.arange(B) % num                                 # neighbouring rows differ
        else:
            mem = np.full(B, int(rng.integers(0, num)))              # one member
        rows, tiles, spans = tile_order(hooks, rates[:num], mem, tpr, grid)
        # a permutation of all (row, tile) pairs
        assert sorted(zip(rows.tolist(), tiles.tolist())) == [(b, t) for b in range(B) for t in range(tpr)]
        # tiles of a member are contiguous: along the list the member never comes back
        along = np.asarray(mem, dtype=np.int64)[rows] if total else np.zeros(0, dtype=np.int64)
        runs = along[np.r_[True, along[1:] != along[:-1]]] if total else along
        assert len(set(runs.tolist())) == runs.size
        # the spans partition the list, each one contiguous: begin(0) = 0, begin(grid) = total, non-decreasing
        assert spans[0] == 0 and spans[grid] == total and (np.diff(spans) >= 0).all()
        sizes = np.diff(spans)
        assert sizes.max() - sizes.min() <= 1      # ... and even
        present = len(set(mem.tolist()))
        for w in range(grid):
            part = along[spans[w]:spans[w + 1]]
            ch = int((part[1:] != part[:-1]).sum())
            assert ch <= max(present - 1, 0) <= num - 1
            changes_seen += ch
        cases += 1
    assert cases == 300 and changes_seen > 100                       # (spans that do change member were among them)
