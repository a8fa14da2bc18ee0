#!/usr/bin/env python3
"""Generate tests/golden/fsmn_memory_golden.npz from the live reference: wekws.model.fsmn.FSMNBlock on the CPU, forward and
autograd, in float32 and in float64, for the golden cases of tests/fsmn_memory_matrix.py.

Per case:
    <name>/x, g, wl, wr            the seeded inputs (float32), as tests/fsmn_memory_matrix.load_case makes them
    <name>/y32, cache32            the float32 block's output and out_cache
    <name>/dx32, dwl32, dwr32      its autograd gradients for the upstream gradient g (not for the forward-only case)
    <name>/y64, dx64, dwl64, dwr64 the same block in float64
and the state-dict keys and shapes of the reference's FSMN for the tiny configuration of tests/test_hip_fsmn_train.py
(fsmn_tiny/keys, fsmn_tiny/shapes) and for fsmn_ctc.yaml's (fsmn_ctc/keys, fsmn_ctc/shapes).
Build container only (needs the reference tree).

    python tests/golden/make_fsmn_memory_golden.py        (from the repository root)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, "/root/reference")
from wekws.model import fsmn as ref_fsmn  # noqa: E402

from tests import fsmn_memory_matrix as fm  # noqa: E402

TINY = (20, 12, 2, 16, 8, 3, 1, 1, 1, 12, 7)
CTC = (400, 140, 4, 250, 128, 10, 2, 1, 1, 140, 2599)


def run(c, dtype):
    D, lorder, rorder = c["x"].shape[2], c["wl"].shape[1], c["wr"].shape[1]
    block = ref_fsmn.FSMNBlock(D, D, lorder, rorder, c["lstride"], c["rstride"]).to(dtype)
    with torch.no_grad():
        block.conv_left.weight.copy_(torch.from_numpy(c["wl"]).to(dtype).view(D, 1, lorder, 1))
        block.conv_right.weight.copy_(torch.from_numpy(c["wr"]).to(dtype).view(D, 1, rorder, 1))
    x = torch.from_numpy(c["x"]).to(dtype).requires_grad_()
    y, cache = block((x, torch.zeros(0, 0, 0, 0, dtype=dtype)))
    out = {"y": y.detach().numpy(), "cache": cache.detach().numpy()}
    if c["backward"]:
        y.backward(torch.from_numpy(c["g"]).to(dtype))
        out.update(dx=x.grad.numpy(), dwl=block.conv_left.weight.grad.numpy().reshape(D, lorder),
                   dwr=block.conv_right.weight.grad.numpy().reshape(D, rorder))
    return out


def main():
    torch.manual_seed(0)
    out = {}
    for name in fm.GOLDEN:
        c = fm.load_case(name)
        for k in ("x", "g", "wl", "wr"):
            out[f"{name}/{k}"] = c[k]
        r32, r64 = run(c, torch.float32), run(c, torch.float64)
        out[f"{name}/cache32"] = r32.pop("cache")
        r64.pop("cache")
        for k, v in r32.items():
            out[f"{name}/{k}32"] = v
        for k, v in r64.items():
            out[f"{name}/{k}64"] = v
        u, bad = fm.units(name, {k: v for k, v in r32.items()})
        print(f"{name}: reference float32 units {u} class mismatches {bad}")
    for tag, cfg in (("fsmn_tiny", TINY), ("fsmn_ctc", CTC)):
        sd = ref_fsmn.FSMN(*cfg).state_dict()
        out[f"{tag}/keys"] = np.array(list(sd))
        out[f"{tag}/shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    path = os.path.join(HERE, "fsmn_memory_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
