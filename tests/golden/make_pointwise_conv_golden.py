#!/usr/bin/env python3
"""Generate tests/golden/pointwise_conv_golden.npz from the live reference: the pointwise convolutions of wekws.model.tcn and
wekws.model.mdtc on the CPU, forward and autograd, in float32 and in float64, for the golden cases of
tests/pointwise_conv_matrix.py (GOLDEN: case -> module):

    ds           DsCnnBlock(C, 3, 1).cnn[3]
    tcnblock     TCNBlock(C, C, 3, 1, True).conv2
    dsd          DSDilatedConv1d(Ci, Co, 3).pointwise, Ci != Co
    dsd_nobias   DSDilatedConv1d(Ci, Co, 3, bias=False).pointwise

Per case:
    <name>/x, g, w[, bias]         the seeded inputs (float32), as tests/pointwise_conv_matrix.load_case makes them
    <name>/y32, dx32, dw32[, db32] the float32 convolution's output and its autograd gradients for the upstream gradient g
    <name>/y64, dx64, dw64[, db64] the same convolution in float64
Only arrays.  Build container only (needs the reference tree).

    python tests/golden/make_pointwise_conv_golden.py        (from the repository root)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, "/root/reference")
from wekws.model import mdtc as ref_mdtc  # noqa: E402
from wekws.model import tcn as ref_tcn  # noqa: E402

from tests import pointwise_conv_matrix as pm  # noqa: E402


def module(kind, Ci, Co):
    if kind == "ds":
        assert Ci == Co
        return ref_tcn.DsCnnBlock(Ci, 3, 1).cnn[3]
    if kind == "tcnblock":
        assert Ci == Co
        return ref_mdtc.TCNBlock(Ci, Ci, 3, 1, True).conv2
    if kind == "dsd":
        assert Ci != Co
        return ref_mdtc.DSDilatedConv1d(Ci, Co, 3).pointwise
    assert kind == "dsd_nobias"
    return ref_mdtc.DSDilatedConv1d(Ci, Co, 3, bias=False).pointwise


def run(c, kind, dtype):
    Co, Ci = c["w"].shape
    conv = module(kind, Ci, Co).to(dtype)
    assert tuple(conv.weight.shape) == (Co, Ci, 1) and (conv.bias is None) == (c["bias"] is None)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(c["w"].copy()).to(dtype).view(Co, Ci, 1))
        if c["bias"] is not None:
            conv.bias.copy_(torch.from_numpy(c["bias"].copy()).to(dtype))
    x = torch.from_numpy(c["x"].copy()).to(dtype).requires_grad_()
    y = conv(x)
    y.backward(torch.from_numpy(c["g"].copy()).to(dtype))
    out = dict(y=y.detach().numpy(), dx=x.grad.numpy(), dw=conv.weight.grad.numpy().reshape(Co, Ci))
    if c["bias"] is not None:
        out["db"] = conv.bias.grad.numpy()
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    out = {}
    for name, kind in pm.GOLDEN.items():
        c = pm.load_case(name)
        for k in ("x", "g", "w", "bias"):
            if c[k] is not None:
                out[f"{name}/{k}"] = c[k]
        r32, r64 = run(c, kind, torch.float32), run(c, kind, torch.float64)
        for k, v in r32.items():
            out[f"{name}/{k}32"] = v
        for k, v in r64.items():
            out[f"{name}/{k}64"] = v
        u, bad = pm.units(name, r32)
        print(f"{name} ({kind}): reference float32 units {u} class mismatches {bad}")
    path = os.path.join(HERE, "pointwise_conv_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
