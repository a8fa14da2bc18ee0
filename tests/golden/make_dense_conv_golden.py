#!/usr/bin/env python3
"""Generate tests/golden/dense_conv_golden.npz from the live reference: the dense convolutions of wekws.model.tcn and
wekws.model.subsampling on the CPU, forward and autograd, in float32 and in float64, for the golden cases of
tests/dense_conv_matrix.py (GOLDEN: case -> module):

    cnn            CnnBlock(C, K, d).cnn[0] behind the block's own F.pad(x, (block.padding, 0))
    subsampling1   Conv1dSubsampling1(Ci, Co).out[0], no padding

Per case:
    <name>/x, g, w, bias           the seeded inputs (float32), as tests/dense_conv_matrix.load_case makes them
    <name>/y32, dx32, dw32, db32   the float32 convolution's output and its autograd gradients for the upstream gradient g
    <name>/y64, dx64, dw64, db64   the same convolution in float64
and the state-dict layouts the swap is tested on, lists of names and shapes:
    tcn_cnn/keys, shapes           TCN(4, 64, 8, block_class=CnnBlock)
    subsampling1/keys, shapes      Conv1dSubsampling1(40, 64)
Only arrays.  Needs the reference tree:

    WEKWS_REFERENCE=<reference checkout> python tests/golden/make_dense_conv_golden.py        (from the repository root)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
if not os.environ.get("WEKWS_REFERENCE"):
    sys.exit("set WEKWS_REFERENCE to a checkout of the reference")
sys.path.insert(0, os.environ["WEKWS_REFERENCE"])
from wekws.model import subsampling as ref_sub  # noqa: E402
from wekws.model import tcn as ref_tcn  # noqa: E402

from tests import dense_conv_matrix as dm  # noqa: E402


def module(kind, s):
    """-> (the convolution, the padding the reference puts in front of it)."""
    if kind == "cnn":
        assert s["Ci"] == s["Co"]
        block = ref_tcn.CnnBlock(s["Ci"], s["K"], s["d"])
        return block.cnn[0], block.padding
    assert kind == "subsampling1"
    return ref_sub.Conv1dSubsampling1(s["Ci"], s["Co"]).out[0], 0


def run(c, kind, dtype):
    s = c["spec"]
    conv, padding = module(kind, s)
    conv = conv.to(dtype)
    assert tuple(conv.weight.shape) == c["w"].shape and conv.dilation == (s["d"],) and padding == s["P"]
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(c["w"].copy()).to(dtype))
        conv.bias.copy_(torch.from_numpy(c["bias"].copy()).to(dtype))
    x = torch.from_numpy(c["x"].copy()).to(dtype).requires_grad_()
    y = conv(F.pad(x, (padding, 0), value=0.0))
    y.backward(torch.from_numpy(c["g"].copy()).to(dtype))
    return dict(y=y.detach().numpy(), dx=x.grad.numpy(), dw=conv.weight.grad.numpy(), db=conv.bias.grad.numpy())


def layout(model):
    sd = model.state_dict()
    return np.array(list(sd)), np.array([",".join(str(d) for d in v.shape) for v in sd.values()])


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    out = {}
    for name, kind in dm.GOLDEN.items():
        c = dm.load_case(name)
        for k in ("x", "g", "w", "bias"):
            out[f"{name}/{k}"] = c[k]
        r32, r64 = run(c, kind, torch.float32), run(c, kind, torch.float64)
        for k, v in r32.items():
            out[f"{name}/{k}32"] = v
        for k, v in r64.items():
            out[f"{name}/{k}64"] = v
        u, bad = dm.units(name, r32)
        print(f"{name} ({kind}): reference float32 units {u} class mismatches {bad}")
    out["tcn_cnn/keys"], out["tcn_cnn/shapes"] = layout(ref_tcn.TCN(4, 64, 8, block_class=ref_tcn.CnnBlock))
    out["subsampling1/keys"], out["subsampling1/shapes"] = layout(ref_sub.Conv1dSubsampling1(40, 64))
    path = os.path.join(HERE, "dense_conv_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
