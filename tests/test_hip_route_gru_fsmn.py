"""GPU: the GRU and FSMN routes of the recipe calls (tests/route_matrix.py: GRU_CALLS, FSMN_CALLS) on the device.  A child process
with the TEST build of the library (libwekws_hip_hooks.so: its route trace) runs each call -- tests/tools/route_gru_fsmn_cases.py --
and the trace of the forward must be the route route.h predicts on the CPU (wekws_hip_debug_gru_route / _fsmn_route), the launch
that ran and not a neighbour: the GRU's family, tiles, slots, variant and where its non-finite pass ran; every FSMN tile's frame
tiles, utterances per workgroup, head slices, grid and LDS."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from tests import route_matrix as rm
from wekws_amd.utils import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "tools", "route_gru_fsmn_cases.py")


@pytest.fixture(scope="module")
def traces():
    hooks = rm.hooks_path()
    assert os.path.exists(hooks), f"{hooks} is missing: make -C wekws_amd/csrc hooks (or __graft_entry__.build())"
    env = dict(os.environ, WEKWS_HIP_LIB=hooks)
    r = subprocess.run([sys.executable, CASES], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    return {(d["model"], d["B"], d["T"]): d for d in map(json.loads, (l for l in r.stdout.splitlines() if l.startswith("{")))}


@pytest.mark.parametrize("name,B,T", rm.GRU_CALLS + rm.FSMN_CALLS)
def test_traced_route_is_route_h(traces, name, B, T):
    lib = rm.type_hooks(C.CDLL(rm.hooks_path()))
    cfg = synth.MODEL_CONFIGS[name]
    d = traces[(name, B, T)]
    if cfg["backbone"]["type"] == "gru":
        r = rm.gru_route(lib, cfg, B, T, cus=d["cus"])
        want = [rm.GRU_FAMILIES.index(r["family"])] + rm.gru_record(r)[1:]
        assert d["path"] == 3 and d["records"] == [want], (d, want)
    else:
        want = []
        for i in range(d["ntiles"]):
            want.append(rm.fsmn_record(rm.fsmn_route(lib, cfg, B, T, tile=i, cus=d["cus"])))
        assert d["path"] == 4 and d["records"] == want, (d, want)
