"""CPU: the host-only entry points of the global CMVN statistics -- wekws_hip_cmvn_stats_plan against a Python restatement of
csrc/cmvn_stats_plan.h, and the refusals of wekws_hip_cmvn_stats_create that need no device."""
import ctypes as C

import pytest

from wekws_amd import _capi

TILE_FLOATS = 8192
FOLD_SEG = 64
DIMS = (1, 40, 80, 83, 400, 4096)


def plan(B, T, D):
    """frames a tile holds (from D alone), tiles of the B * T frames numbered row by row, bytes of scratch: 2 D doubles a tile
    and, where there are more than FOLD_SEG tiles, 2 D doubles per FOLD_SEG tiles for the first stage of the fold"""
    tile = max(1, TILE_FLOATS // D)
    tiles = -(-(B * T) // tile)
    segments = -(-tiles // FOLD_SEG) if tiles > FOLD_SEG else 0
    return [tile, tiles, (tiles + segments) * 2 * D * 8]


@pytest.mark.parametrize("D", DIMS)
def test_plan_equals_its_restatement(D):
    lib = _capi.load()
    out = (C.c_int64 * 3)()
    tile = plan(1, 1, D)[0]
    for B in range(6):
        for T in range(2 * tile + 2):
            assert lib.wekws_hip_cmvn_stats_plan(B, T, D, out) == 0, _capi.last_error()
            assert list(out) == plan(B, T, D), (B, T, D)


def tile_of(D):
    return plan(1, 1, D)[0]


def test_plan_does_not_depend_on_anything_but_the_shape():
    """the tile is a function of D; a shape's tiles cover its frames exactly once"""
    lib = _capi.load()
    out = (C.c_int64 * 3)()
    for D in DIMS:
        tiles = set()
        for B, T in ((1, 1), (5, 98), (1024, 98), (3, 100000), (65, tile_of(D)), (64, tile_of(D))):
            assert lib.wekws_hip_cmvn_stats_plan(B, T, D, out) == 0
            tiles.add(out[0])
            assert (out[1] - 1) * out[0] < B * T <= out[1] * out[0]
            assert list(out) == plan(B, T, D)
        assert len(tiles) == 1


def test_plan_refuses_bad_shapes():
    lib = _capi.load()
    out = (C.c_int64 * 3)()
    for B, T, D in ((1, 1, 0), (1, 1, 4097), (-1, 1, 80), (1, -1, 80), (65536, 32768, 80)):
        assert lib.wekws_hip_cmvn_stats_plan(B, T, D, out) == -1, (B, T, D)
        assert _capi.last_error() != ""
    assert lib.wekws_hip_cmvn_stats_plan(1, 1, 80, None) == -1
    assert lib.wekws_hip_cmvn_stats_plan(65536, 32767, 80, out) == 0          # 2^31 - 65536 frames: the most a call takes


def test_create_checks_dim_before_the_device():
    lib = _capi.load()
    for dim in (0, 4097, -3):
        h = C.c_void_p()
        assert lib.wekws_hip_cmvn_stats_create(dim, 0, C.byref(h)) == -1 and not h
        assert "dim" in _capi.last_error()
    assert lib.wekws_hip_cmvn_stats_create(80, 0, None) == -1


def test_create_without_a_gpu_is_edevice():
    import torch
    h = C.c_void_p()
    lib = _capi.load()
    if torch.cuda.is_available():
        assert lib.wekws_hip_cmvn_stats_create(80, torch.cuda.device_count(), C.byref(h)) == -3 and not h      # no such device
    else:
        assert lib.wekws_hip_cmvn_stats_create(80, 0, C.byref(h)) == -3 and not h
    assert _capi.last_error() != ""


def test_handle_calls_reject_null():
    lib = _capi.load()
    counts = (C.c_int64 * 2)()
    assert lib.wekws_hip_cmvn_stats_update(None, None, 1, 1, None, None) == -1 and "NULL" in _capi.last_error()
    assert lib.wekws_hip_cmvn_stats_reset(None, None) == -1
    assert lib.wekws_hip_cmvn_stats_read(None, None, None, counts, None) == -1
    lib.wekws_hip_cmvn_stats_destroy(None)
