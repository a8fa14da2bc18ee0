#!/usr/bin/env python3
"""Generate tests/golden/depthwise_conv_golden.npz from the live reference: the depthwise convolutions of wekws.model.tcn and
wekws.model.mdtc on the CPU, forward and autograd, in float32 and in float64, for the golden cases of
tests/depthwise_conv_matrix.py, and the reference's backbones for the module mirrors of wekws_amd.model.tcn / .mdtc.

Per case (a case with a bias runs ``DsCnnBlock(C, K, d).cnn[0]``, one without ``DSDilatedConv1d(C, C, K, d, bias=False).conv``,
both behind ``F.pad(x, (P, 0))``):
    <name>/x, g, w[, bias]         the seeded inputs (float32), as tests/depthwise_conv_matrix.load_case makes them
    <name>/y32                     the float32 convolution's output
    <name>/dx32, dw32[, db32]      its autograd gradients for the upstream gradient g (not for the forward-only case)
    <name>/y64, dx64, dw64[, db64] the same convolution in float64
Per model tag -- tcn_ds (TCN(4, 64, 8, block_class=DsCnnBlock)), tcn_tiny_ds and tcn_tiny_cnn (TCN(2, 8, 3, ...) in both
block classes), mdtc_small (MDTC(3, 4, 80, 32, 5, True)), mdtc_tiny (MDTC(2, 2, 6, 8, 3, True)) and mdtc_tiny_sq
(MDTC(2, 2, 8, 8, 3, True)):
    <tag>/keys, <tag>/shapes       the state-dict keys and shapes
and for tcn_tiny_ds, tcn_tiny_cnn and mdtc_tiny_sq, in eval() with a seeded state dict:
    <tag>/sd/<key>                 the state dict
    <tag>/x                        an input (3, 11, D)
    <tag>/y, <tag>/cache           the backbone's output and cache for an empty cache
    <tag>/y1, cache1, y2, cache2   the same input in two chunks (frames 0..4, 5..10) with the carried cache
Build container only (needs the reference tree).

    python tests/golden/make_depthwise_conv_golden.py        (from the repository root)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, "/root/reference")
from wekws.model import mdtc as ref_mdtc  # noqa: E402
from wekws.model import tcn as ref_tcn  # noqa: E402

from tests import depthwise_conv_matrix as dm  # noqa: E402

MODELS = {
    "tcn_ds": lambda: ref_tcn.TCN(4, 64, 8, block_class=ref_tcn.DsCnnBlock),
    "tcn_tiny_ds": lambda: ref_tcn.TCN(2, 8, 3, block_class=ref_tcn.DsCnnBlock),
    "tcn_tiny_cnn": lambda: ref_tcn.TCN(2, 8, 3, block_class=ref_tcn.CnnBlock),
    "mdtc_small": lambda: ref_mdtc.MDTC(3, 4, 80, 32, 5, True),
    "mdtc_tiny": lambda: ref_mdtc.MDTC(2, 2, 6, 8, 3, True),
    "mdtc_tiny_sq": lambda: ref_mdtc.MDTC(2, 2, 8, 8, 3, True),
}
# tag -> input dimension.  (The reference's MDTC.forward concatenates the preprocessor's cache, of in_channels channels, with
# the stacks', of res_channels: it runs only where the two are equal, as init_model builds it.  mdtc_small and mdtc_tiny above
# are recorded for their keys and shapes; the forward goldens take the square mdtc_tiny_sq.)
TINY = {"tcn_tiny_ds": 8, "tcn_tiny_cnn": 8, "mdtc_tiny_sq": 8}


def run(c, dtype):
    C, K = c["w"].shape
    if c["bias"] is not None:
        conv = ref_tcn.DsCnnBlock(C, K, c["d"]).cnn[0]
    else:
        conv = ref_mdtc.DSDilatedConv1d(C, C, K, dilation=c["d"], bias=False).conv
    conv = conv.to(dtype)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(c["w"]).to(dtype).view(C, 1, K))
        if c["bias"] is not None:
            conv.bias.copy_(torch.from_numpy(c["bias"]).to(dtype))
    x = torch.from_numpy(c["x"]).to(dtype).requires_grad_()
    y = conv(F.pad(x, (c["P"], 0), value=0.0))
    out = {"y": y.detach().numpy()}
    if c["backward"]:
        y.backward(torch.from_numpy(c["g"]).to(dtype))
        out.update(dx=x.grad.numpy(), dw=conv.weight.grad.numpy().reshape(C, K))
        if c["bias"] is not None:
            out["db"] = conv.bias.grad.numpy()
    return out


def seed_state(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith("running_var"):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
            elif k.endswith("num_batches_tracked"):
                continue
            else:
                v.copy_(0.3 * torch.randn(v.shape, generator=g))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    out = {}
    for name in dm.GOLDEN:
        c = dm.load_case(name)
        for k in ("x", "g", "w", "bias"):
            if c[k] is not None:
                out[f"{name}/{k}"] = c[k]
        r32, r64 = run(c, torch.float32), run(c, torch.float64)
        for k, v in r32.items():
            out[f"{name}/{k}32"] = v
        for k, v in r64.items():
            out[f"{name}/{k}64"] = v
        u, bad = dm.units(name, r32)
        print(f"{name}: reference float32 units {u} class mismatches {bad}")
    for i, (tag, make) in enumerate(MODELS.items()):
        model = make().eval()
        sd = model.state_dict()
        out[f"{tag}/keys"] = np.array(list(sd))
        out[f"{tag}/shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        if tag not in TINY:
            continue
        seed_state(model, 100 + i)
        for k, v in model.state_dict().items():
            out[f"{tag}/sd/{k}"] = v.numpy().copy()
        x = torch.randn(3, 11, TINY[tag], generator=torch.Generator().manual_seed(200 + i))
        with torch.no_grad():
            y, cache = model(x)
            y1, cache1 = model(x[:, :5])
            y2, cache2 = model(x[:, 5:], cache1)
        for k, v in dict(x=x, y=y, cache=cache, y1=y1, cache1=cache1, y2=y2, cache2=cache2).items():
            out[f"{tag}/{k}"] = v.numpy().copy()
    path = os.path.join(HERE, "depthwise_conv_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
