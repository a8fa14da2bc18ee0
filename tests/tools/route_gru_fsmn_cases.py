"""Runs the GRU and FSMN recipe calls of tests/route_matrix.py (GRU_CALLS, FSMN_CALLS) on the GPU with the TEST build of the library
(libwekws_hip_hooks.so, for wekws_hip_debug_route_trace), for tests/test_hip_route_gru_fsmn.py.  Run as a subprocess with
WEKWS_HIP_LIB pointing at it.  One JSON line per call: the trace's path and records; then OK."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import route_matrix as rm  # noqa: E402
from wekws_amd import _capi, pack  # noqa: E402
from wekws_amd.model.kws_model import init_model  # noqa: E402
from wekws_amd.utils import synth  # noqa: E402

MAX = 8


def main():
    lib = rm.type_hooks(_capi.load())
    assert _capi.lib_path().endswith("libwekws_hip_hooks.so"), _capi.lib_path()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    models = {}
    for name, B, T in rm.GRU_CALLS + rm.FSMN_CALLS:
        cfg = synth.MODEL_CONFIGS[name]
        if name not in models:
            sd = synth.synth_state_dict(pack.model_spec(cfg), 1234)
            m = init_model(cfg)
            m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
            models[name] = m.cuda().eval()
        x = torch.from_numpy(synth.synth_feats(B, T, cfg["input_dim"], seed=3)).cuda()
        models[name](x)
        torch.cuda.synchronize()
        out = (ctypes.c_int * (2 + 9 * MAX))()
        n = lib.wekws_hip_debug_route_trace(out, MAX)
        recs = [list(out[2 + 9 * i:11 + 9 * i]) for i in range(n)]
        print(json.dumps(dict(model=name, B=B, T=T, cus=cus, path=out[0], ntiles=out[1], records=recs)), flush=True)
    print("OK")


if __name__ == "__main__":
    main()
