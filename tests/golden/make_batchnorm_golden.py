#!/usr/bin/env python3
"""Generate tests/golden/batchnorm_golden.npz from the live reference: the BatchNorm sites of wekws.model.tcn and wekws.model.mdtc
on the CPU, forward and autograd, in float32 and in float64, for the golden cases of tests/batchnorm_matrix.py.

The sites, built from the reference's own modules and run by its own statements:
    ds    DsCnnBlock(C, 3, 1).cnn[1:3]                       y = relu(bn(x))
    dsd   DSDilatedConv1d(C, C, 3).bn                        y = bn(x)
    bn1   TCNBlock(C, C, 3, 1, True).bn1, .relu1             y = relu1(bn1(x))
    bn2   TCNBlock(C, C, 3, 1, True).bn2, .relu2             y = relu2(bn2(x) + inputs)
Per case, in train() or eval() as the case says, the module's parameters and buffers set to the case's:
    <name>/x, g[, res], w, b, rm, rv          the seeded inputs (float32), as tests/batchnorm_matrix.load_case makes them
    <name>/y32, dx32, dw32, db32[, dres32]    the float32 site's output and its autograd gradients for the upstream gradient g
    <name>/rm32, rv32, tracked32              the buffers after that one call
    <name>/...64                              the same site in float64
Build container only (needs the reference tree).

    python tests/golden/make_batchnorm_golden.py        (from the repository root)
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

from tests import batchnorm_matrix as bm  # noqa: E402


def site(kind, C):
    """-> (bn, f): the reference's BatchNorm module and the site's statements as f(x, res)."""
    if kind == "ds":
        cnn = ref_tcn.DsCnnBlock(C, 3, 1).cnn
        return cnn[1], lambda x, res: cnn[2](cnn[1](x))
    if kind == "dsd":
        bn = ref_mdtc.DSDilatedConv1d(C, C, 3).bn
        return bn, lambda x, res: bn(x)
    blk = ref_mdtc.TCNBlock(C, C, 3, 1, True)
    if kind == "bn1":
        return blk.bn1, lambda x, res: blk.relu1(blk.bn1(x))
    return blk.bn2, lambda x, res: blk.relu2(blk.bn2(x) + res)


def run(name, dtype):
    c = bm.load_case(name)
    C = c["x"].shape[1]
    bn, f = site(bm.GOLDEN_SITE[name], C)
    bn = bn.to(dtype)
    assert bn.eps == bm.EPS and bn.momentum == c["momentum"]
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(c["w"].copy()).to(dtype))
        bn.bias.copy_(torch.from_numpy(c["b"].copy()).to(dtype))
        bn.running_mean.copy_(torch.from_numpy(c["rm"].copy()).to(dtype))
        bn.running_var.copy_(torch.from_numpy(c["rv"].copy()).to(dtype))
        bn.num_batches_tracked.fill_(c["tracked"])
    bn.train(c["training"])
    x = torch.from_numpy(c["x"].copy()).to(dtype).requires_grad_()
    res = torch.from_numpy(c["res"].copy()).to(dtype).requires_grad_() if c["res"] is not None else None
    y = f(x, res)
    y.backward(torch.from_numpy(c["g"].copy()).to(dtype))
    out = dict(y=y.detach().numpy(), dx=x.grad.numpy(), dw=bn.weight.grad.numpy(), db=bn.bias.grad.numpy(),
               rm=bn.running_mean.numpy().copy(), rv=bn.running_var.numpy().copy(), tracked=np.array(int(bn.num_batches_tracked)))
    if res is not None:
        out["dres"] = res.grad.numpy()
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    out = {}
    for name in bm.GOLDEN:
        c = bm.load_case(name)
        for k in ("x", "g", "res", "w", "b", "rm", "rv"):
            if c[k] is not None:
                out[f"{name}/{k}"] = c[k]
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            for k, v in run(name, dtype).items():
                out[f"{name}/{k}{tag}"] = v
    path = os.path.join(HERE, "batchnorm_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
