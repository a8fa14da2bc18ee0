#!/usr/bin/env python3
"""Generate tests/golden/criterion_grad_golden.npz from the live reference: the gradient torch's autograd gives for
wekws.model.loss.criterion with respect to its input, for every case of tests/criterion_grad_matrix.py.

Per case:
    <name>/grad64        the float64 autograd gradient (inputs cast to float64), cases of at most SMALL elements
    <name>/grad64_sum    its sum over the finite elements, and <name>/oracle_dev the worst deviation of the float64 oracle
                         (tests/criterion_grad_ref.py) from it, in the measure of test_criterion_grad_oracle.py -- larger cases
    <name>/nan32, zero32 the class map of the reference's float32 gradient, bit-packed
    <name>/rows64        ctc: the float64 per-row losses
and per kind <kind>/ref_units: the worst error of the reference's float32 gradient against the float64 oracle in the units of
tests/criterion_grad_matrix.py, from which the bars follow; REF_UNITS and BARS of that file are rewritten from the measurement.

The max-pooling decisions (ties, the clamp's gate) are float32 comparisons; in float64 `1 - x` and the bound 1e-8 are other
numbers, so grad64 is compared only where its class equals the float32 gradient's (the case mpg_ties_6x4x2 holds such a frame),
and in the columns that pool 1 - x to 2^-23 relative (criterion_grad_matrix.MP_OTHER_TOL) where the keyword columns are held to 1e-12.
Build container only (needs /root/reference).

    python tests/golden/make_criterion_grad_golden.py        (from the repository root)
"""
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, "/root/reference")
from wekws.model import loss as ref_loss  # noqa: E402

from tests import criterion_grad_matrix as gm  # noqa: E402
from tests import criterion_grad_ref as gr  # noqa: E402
from tests.helpers import pow2_at_or_above  # noqa: E402


def reference_grad(kind, c, dtype):
    if kind == "max_pooling":
        x = torch.from_numpy(c["scores"]).to(dtype).requires_grad_()
        ln = torch.from_numpy(c["lengths"])
        assert int(ln.max()) == x.size(1)
        loss, _ = ref_loss.criterion("max_pooling", x, torch.from_numpy(c["target"]), ln, min_duration=c["min_duration"])
    elif kind == "ce":
        x = torch.from_numpy(c["logits"]).to(dtype).requires_grad_()
        loss, _ = ref_loss.criterion("ce", x, torch.from_numpy(c["target"]), None)
    else:
        x = torch.from_numpy(c["logits"]).to(dtype).requires_grad_()
        loss, _ = ref_loss.criterion("ctc", x, torch.from_numpy(c["targets"]).long(), torch.from_numpy(c["lengths"]).long(),
                                     target_lengths=torch.from_numpy(c["target_lengths"]).long(), validation=False)
    loss.backward()
    return x.grad.numpy()


def oracle(kind, c, divisor):
    if kind == "max_pooling":
        return gr.max_pooling_grad(c["scores"], c["target"], c["lengths"], c["min_duration"], divisor=divisor), None
    if kind == "ce":
        return gr.cross_entropy_grad(c["logits"], c["target"], divisor=divisor), None
    o = gr.ctc_grad(c["logits"], c["targets"], c["lengths"], c["target_lengths"], divisor=divisor)
    return o["grad"], o["rows"]


def deviation(kind, got, ref, divisor, rows, where=None):
    """max |got - ref| / max(|ref|, scale) over the elements of equal class; scale as the units' denominators."""
    same = gm.classes(got) == gm.classes(ref)
    if where is not None:
        same = same & where
    fin = same & np.isfinite(ref)
    scale = np.full(ref.shape, 1.0 / divisor)
    if kind == "ctc":
        nll = np.where(np.isfinite(rows), np.maximum(1.0, rows), 1.0)
        scale = scale * nll.reshape((-1,) + (1,) * (ref.ndim - 1))
    d = np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)) / np.maximum(np.where(fin, np.abs(ref), 0.0), scale)
    return float(d.max())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    out, worst = {}, {}
    for kind in ("max_pooling", "ce", "ctc"):
        worst[kind] = (0.0, "")
        for name in gm.case_names(kind):
            c = gm.load_case(kind, name)
            B = gm.batch_size(kind, c)
            g32 = reference_grad(kind, c, torch.float32)
            g64 = reference_grad(kind, c, torch.float64)
            o, rows = oracle(kind, c, B)
            cls32 = gm.classes(g32)
            assert np.array_equal(cls32, gm.classes(o)), (name, np.argwhere(cls32 != gm.classes(o))[:5])
            if kind != "max_pooling":
                assert np.array_equal(cls32, gm.classes(g64)), name
            if kind == "max_pooling":
                kw = gm.keyword_columns(c)
                dev = deviation(kind, o, g64, B, rows, kw)
                assert deviation(kind, o, g64, B, rows, ~kw) <= gm.MP_OTHER_TOL, name
            else:
                dev = deviation(kind, o, g64, B, rows)
            assert dev <= 1e-12, (name, dev)
            u = gm.units(kind, g32, o, B, rows)
            if u > worst[kind][0]:
                worst[kind] = (u, name)
            out[name + "/nan32"] = np.packbits(cls32.reshape(-1) == 2)
            out[name + "/zero32"] = np.packbits(cls32.reshape(-1) == 1)
            if g64.size <= gm.SMALL:
                out[name + "/grad64"] = g64
            else:
                out[name + "/grad64_sum"] = np.float64(g64[np.isfinite(g64)].sum())
                out[name + "/oracle_dev"] = np.float64(dev)
            if rows is not None:
                out[name + "/rows64"] = rows
            print(f"{name:18s} B {B:3d} oracle dev {dev:.2e}  ref f32 units {u:.2f}  nan {int((cls32 == 2).sum())} zero {int((cls32 == 1).sum())}")
    lines = {}
    for kind, (u, name) in worst.items():
        out[kind + "/ref_units"] = np.float64(u)
        lines[kind] = (round(u, 2), pow2_at_or_above(4 * u))
        print(f"{kind}: reference's worst error {u:.3f} units ({name}) -> bar {lines[kind][1]}")
    path = os.path.join(HERE, "criterion_grad_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    mpath = os.path.join(HERE, "..", "criterion_grad_matrix.py")
    src = open(mpath).read()
    src = re.sub(r"^REF_UNITS = \{[^}]*\}", "REF_UNITS = {" + ", ".join(f'"{k}": {v[0]}' for k, v in lines.items()) + "}", src, flags=re.M)
    src = re.sub(r"^BARS = \{[^}]*\}", "BARS = {" + ", ".join(f'"{k}": {float(v[1])}' for k, v in lines.items()) + "}", src, flags=re.M)
    open(mpath, "w").write(src)


if __name__ == "__main__":
    main()
