"""CPU: the host side of the streaming threshold detector (wekws_hip_threshold_kws_*) and of the MFCC mode of the streaming
front end (wekws_hip_stream_frontend_create_mfcc): the symbols are exported and bound, bad configurations are refused with
EINVAL and a message before any device work, and a valid one gets as far as the device (EDEVICE without a GPU)."""
import ctypes as C

import pytest
import torch

from tests.test_stream_frontend_plan import make_cfg
from wekws_amd import _capi

EINVAL, EDEVICE = -1, -3
NEW = ("wekws_hip_stream_frontend_create_mfcc", "wekws_hip_threshold_kws_create", "wekws_hip_threshold_kws_destroy",
       "wekws_hip_threshold_kws_max_hits", "wekws_hip_threshold_kws_step", "wekws_hip_threshold_kws_reset",
       "wekws_hip_threshold_kws_state")


def test_new_symbols_are_exported_and_bound():
    lib = _capi.load()
    for name in NEW:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert C.sizeof(_capi.ThresholdKwsSlot) == 16
    assert C.sizeof(_capi.StreamFrontendCfg) == 64            # MFCC mode is an entry point, not a field


def refused(rc):
    return rc == EINVAL and _capi.last_error() != ""


def valid(rc, h, destroy):
    """A valid configuration: created where there is a device, EDEVICE where there is none."""
    if torch.cuda.is_available():
        assert rc == 0 and h, _capi.last_error()
        destroy(h)
    else:
        assert rc == EDEVICE and not h, (rc, _capi.last_error())


def test_create_mfcc_refuses_bad_cepstra_before_the_device():
    lib = _capi.load()
    h = C.c_void_p()
    cfg = make_cfg(bins=40)
    for nc in (0, 41, -1):
        assert refused(lib.wekws_hip_stream_frontend_create_mfcc(C.byref(cfg), nc, 22.0, C.byref(h))) and not h, nc
        assert "num_ceps" in _capi.last_error()
    assert refused(lib.wekws_hip_stream_frontend_create_mfcc(C.byref(cfg), 13, -1.0, C.byref(h))) and not h
    assert refused(lib.wekws_hip_stream_frontend_create_mfcc(C.byref(make_cfg(bins=129)), 13, 22.0, C.byref(h))) and not h
    assert refused(lib.wekws_hip_stream_frontend_create_mfcc(None, 13, 22.0, C.byref(h)))
    assert refused(lib.wekws_hip_stream_frontend_create_mfcc(C.byref(cfg), 13, 22.0, None))
    # what wekws_hip_stream_frontend_create refuses is refused here too
    assert refused(lib.wekws_hip_stream_frontend_create_mfcc(C.byref(make_cfg(bins=40, left=1, right=2)), 13, 22.0, C.byref(h)))
    for nc, q in ((13, 22.0), (40, 0.0), (1, 22.0)):
        rc = lib.wekws_hip_stream_frontend_create_mfcc(C.byref(cfg), nc, q, C.byref(h))
        valid(rc, h, lib.wekws_hip_stream_frontend_destroy)
        h = C.c_void_p()
    # the reserved words stay ignored, in both modes
    cfg.reserved[0], cfg.reserved[1] = 80, -7
    rc = lib.wekws_hip_stream_frontend_create_mfcc(C.byref(cfg), 13, 22.0, C.byref(h))
    valid(rc, h, lib.wekws_hip_stream_frontend_destroy)


def test_threshold_create_refuses_bad_arguments_before_the_device():
    lib = _capi.load()
    h = C.c_void_p()
    th = (C.c_double * 2)(0.5, 0.25)
    bad = [dict(K=0), dict(K=-1), dict(ws=0), dict(ws=-3), dict(streams=0), dict(th=None)]
    for kw in bad:
        a = dict(K=2, th=th, ws=50, streams=4)
        a.update(kw)
        assert refused(lib.wekws_hip_threshold_kws_create(a["K"], a["th"], a["ws"], a["streams"], 0, C.byref(h))) and not h, kw
    assert "NULL" in _capi.last_error()
    assert refused(lib.wekws_hip_threshold_kws_create(2, th, 50, 4, 0, None))
    rc = lib.wekws_hip_threshold_kws_create(2, th, 50, 4, 0, C.byref(h))
    valid(rc, h, lib.wekws_hip_threshold_kws_destroy)


def test_threshold_entry_points_reject_a_null_handle():
    lib = _capi.load()
    assert lib.wekws_hip_threshold_kws_max_hits(None, 10) == 0
    assert refused(lib.wekws_hip_threshold_kws_step(None, None, 1, 1, None, None, None, None, None, None, None, None))
    assert refused(lib.wekws_hip_threshold_kws_reset(None, None, 0, None))
    assert refused(lib.wekws_hip_threshold_kws_state(None, 0, 0, None, None))
    lib.wekws_hip_threshold_kws_destroy(None)


def test_python_spotter_refuses_bad_settings_without_a_device():
    from wekws_amd.det import StreamingThresholdSpotter
    for kw in (dict(keywords=[], threshold=0.5), dict(keywords=["a", "b"], threshold=[0.1, 0.2, 0.3]),
               dict(keywords=["a"], threshold=0.5, window_shift=0)):
        with pytest.raises(ValueError):
            StreamingThresholdSpotter(4, device="cuda:0", **kw)
