#!/usr/bin/env python3
"""Generate tests/golden/gru_train_golden.npz from the live reference: the backbone of wekws.model.kws_model.init_model for a
small gru config (hidden 16, 2 layers), under its own initialisation, on the CPU: forward and autograd in float32 and in float64.

    x (B, T, H), h0 (L, B, H), gy (B, T, H), ghn (L, B, H)        the seeded inputs and upstream gradients (float32)
    weight_ih_l*, weight_hh_l*, bias_ih_l*, bias_hh_l*             the backbone's parameters as init_model made them
    y32, hn32, dx32, dh032, d<parameter>32                         output, h_n and every gradient of the float32 backbone
    ...64                                                          the same backbone in float64
The loss is sum(y gy) + sum(h_n ghn).  The backbone is given h0 explicitly: the reference's KWSModel.forward passes its empty
default cache on to nn.GRU, which refuses it.  Build container only (needs the reference tree).

    python tests/golden/make_gru_train_golden.py        (from the repository root)
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, "/root/reference")
from wekws.model.kws_model import init_model  # noqa: E402

CONFIG = dict(input_dim=20, output_dim=2, hidden_dim=16, preprocessing=dict(type="linear"), backbone=dict(type="gru", num_layers=2))
B, T = 3, 5


def run(gru, arrays, dtype):
    gru = copy.deepcopy(gru).to(dtype)
    x = torch.from_numpy(arrays["x"]).to(dtype).requires_grad_()
    h0 = torch.from_numpy(arrays["h0"]).to(dtype).requires_grad_()
    y, hn = gru(x, h0)
    ((y * torch.from_numpy(arrays["gy"]).to(dtype)).sum() + (hn * torch.from_numpy(arrays["ghn"]).to(dtype)).sum()).backward()
    out = dict(y=y.detach().numpy(), hn=hn.detach().numpy(), dx=x.grad.numpy(), dh0=h0.grad.numpy())
    for n, p in gru.named_parameters():
        out[f"d{n}"] = p.grad.numpy()
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    model = init_model(CONFIG)
    gru = model.backbone
    assert isinstance(gru, torch.nn.GRU) and gru.batch_first and gru.num_layers == 2 and gru.hidden_size == 16
    rng = np.random.default_rng(0)
    H, L = gru.hidden_size, gru.num_layers
    out = dict(x=rng.standard_normal((B, T, H)).astype(np.float32), h0=rng.standard_normal((L, B, H)).astype(np.float32),
               gy=rng.standard_normal((B, T, H)).astype(np.float32), ghn=rng.standard_normal((L, B, H)).astype(np.float32))
    for n, p in gru.named_parameters():
        out[n] = p.detach().numpy().copy()
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        for k, v in run(gru, out, dtype).items():
            out[f"{k}{tag}"] = v
    path = os.path.join(HERE, "gru_train_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
