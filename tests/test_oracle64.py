"""The float64 mode of the numpy oracle (oracle/kws_oracle.py, dtype=np.float64) against every stored live-reference golden set.
CPU only.  The goldens are the reference's own float32 results, so they differ from the float64 evaluation of the same function by
float32 rounding alone; the bound below is that level, on the scale of the tight bar (tests/helpers.py::tight_error).  This is what
lets the GPU parity tests hold the kernels to a bar tighter than the goldens' own rounding: they compare with this evaluation."""
import os

import numpy as np
import pytest

from oracle import kws_oracle
from tests.golden.cases import (GENERIC_CASES, GRU_INPUT_CASES, HETERO_CASES, SCALE_CASES, SHAPE_CASES, hetero_case_weights,
                                scaled_case_weights, shape_case_config)
from tests.helpers import CASES, case_in_cache, case_input, case_weights, oracle64, tight_errors
from wekws_amd import pack
from wekws_amd.utils import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# float32 rounding through a whole network, in units of the tight bar's scale (per channel for logits / caches, absolute for
# posteriors): measured at most 2.4e-5 over the 223 golden sets below -- the logits of the FSMN CTC heads (300 / 2599 classes), whose
# channels are sums that cancel to a small fraction of their terms --, 8.7e-6 everywhere else.  2^-14 (6.1e-5): float32 rounding
# level, 1.6x below the 1e-4 of the float32 parity tests.
F32_ROUNDING = 2.0 ** -14


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


def _entries():
    out = []
    for c in CASES:
        out.append(("model_golden.npz", c))
    for c in SCALE_CASES:
        out.append(("scale_golden.npz", c))
    for c in HETERO_CASES + GRU_INPUT_CASES:
        out.append(("hetero_golden.npz", c))
    for c in SHAPE_CASES:
        out.append(("shape_golden.npz", c))
    for c in GENERIC_CASES:
        out.append(("generic_golden.npz", c))
    return out


ENTRIES = _entries()


def _case(npz, case):
    """-> cfg, sd, x, in_cache, chunks, softmax, and the goldens (y, cache or None, one-shot-then-two-chunks extras)."""
    g = _load(npz)
    name = case["name"]
    if npz in ("shape_golden.npz", "generic_golden.npz"):
        cfg = shape_case_config(case)
        sd = synth.synth_state_dict(pack.model_spec(cfg), case["wseed"])
        x = synth.synth_feats(case["B"], case["T"], cfg["input_dim"], seed=case["xseed"])
        extra = None
        if case.get("split"):
            extra = ([case["split"], case["T"] - case["split"]], g[name + "/y_stream"], g[name + "/cache_stream"])
        return cfg, sd, x, None, None, False, g[name + "/y"], g[name + "/cache"], extra
    cfg, sd = case_weights(case)
    x = case_input(case)
    if npz == "scale_golden.npz":
        sd, xs = scaled_case_weights(case, sd)
        x = (x * np.float32(xs)).astype(np.float32)
    elif npz == "hetero_golden.npz":
        if case.get("hetero"):
            sd = hetero_case_weights(case, sd)
        x = (x * np.float32(case.get("xscale", 1.0))).astype(np.float32)
    if name + "/wsum" in g.files:
        assert abs(synth.checksum(sd) - float(g[name + "/wsum"])) <= 1e-6 * abs(float(g[name + "/wsum"]))
    gc = g[name + "/cache"] if name + "/cache" in g.files else None
    return cfg, sd, x, case_in_cache(case, cfg), case.get("chunks"), case.get("softmax", False), g[name + "/y"], gc, None


@pytest.mark.parametrize("npz,case", ENTRIES, ids=[f"{n.split('_golden')[0]}/{c['name']}" for n, c in ENTRIES])
def test_float64_oracle_against_every_golden_set(npz, case):
    cfg, sd, x, cache0, chunks, softmax, gy, gc, extra = _case(npz, case)
    ry, rc = oracle64(cfg, sd, x, cache0, chunks, softmax)
    assert ry.dtype == np.float64 and rc.dtype == np.float64
    assert ry.shape == gy.shape
    if gc is not None and rc.shape != gc.shape:
        rc = rc[:1]                                    # (model_golden stores the first utterance's cache of a conv / FSMN model)
    ey, ec = tight_errors(cfg, gy, gc, ry, rc, softmax)
    assert ey <= F32_ROUNDING and ec <= F32_ROUNDING, (ey, ec)
    if extra:
        chunks2, gys, gcs = extra
        rys, rcs = oracle64(cfg, sd, x, None, chunks2)
        assert max(tight_errors(cfg, gys, gcs, rys, rcs)) <= F32_ROUNDING


def test_float32_default_is_unchanged_and_float64_is_a_different_evaluation():
    """dtype defaults to float32 (the restatement the rest of the suite pins against the goldens); float64 is the same
    function, closer to the float32 results than float32 rounding and yet not equal to them."""
    cfg = synth.MODEL_CONFIGS["mdtc_h64"]
    sd = synth.synth_state_dict(pack.model_spec(cfg), 3)
    x = synth.synth_feats(2, 30, cfg["input_dim"], seed=3)
    y, c = kws_oracle.forward(cfg, sd, x)
    y32, c32 = kws_oracle.forward(cfg, sd, x, dtype=np.float32)
    assert y.dtype == np.float32 and np.array_equal(y, y32) and np.array_equal(c, c32)
    y64, c64 = kws_oracle.forward(cfg, sd, x, dtype=np.float64)
    assert y64.dtype == np.float64 and not np.array_equal(y64, y)
    assert float(np.abs(y64 - y).max()) <= 1e-5
    ys, cs = kws_oracle.forward_streaming(cfg, sd, x, [7, 23], dtype=np.float64)
    assert ys.dtype == np.float64 and float(np.abs(ys - y64).max()) <= 1e-12 and float(np.abs(cs - c64).max()) <= 1e-12
