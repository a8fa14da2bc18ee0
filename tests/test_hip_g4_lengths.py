"""Every length through the register-resident kernels of the small recipes (ds64_g4 / mdtc_g4: one utterance per workgroup of
C / 16 waves, the lane-major tile of csrc/lane_tile.hip.h with the utterance's END on a lane boundary): all three models, where
tests/test_hip_parity.py sweeps MDTC h64 without a cache and samples five chunkings with one.
  * without a cache, T = 1 .. 112 against the LDS-tile kernels (option g16 = 0): every `off` = (-T) mod NT in every tile size,
    slices longer than the input, partial lanes in the hand-over.  The bars are the ones of
    test_register_resident_kernels_at_every_length (end-aligned tile: other padding frames, so rounding noise, 3e-6) and of
    test_ds64_register_resident_kernel (posteriors 2e-6);
  * with an incoming cache, a second chunk of T = 17 .. 112 frames on the cache of a 98-frame first chunk, the context variants
    against the LDS-tile kernels (option g16 = 3): every `off`, every slice boundary inside a lane, T < pad for the 28- and
    56-frame paddings.  The assertions of the three ..._with_incoming_cache tests: caches bit for bit, posteriors 5e-7."""
import numpy as np
import pytest

from tests.helpers import max_abs
from tests.test_hip_parity import build, run
from wekws_amd import pack
from wekws_amd.utils import synth

pytestmark = pytest.mark.gpu

B = 2
# (model, output_dim or None = the recipe's, bar on the posteriors without a cache)
MODELS = (("ds_tcn_h64", 2, 2e-6), ("mdtc_h64", None, 3e-6), ("mdtc_small", None, 3e-6))


def _weights(name, odim):
    cfg = dict(synth.MODEL_CONFIGS[name])
    if odim:
        cfg["output_dim"] = odim
    return cfg, synth.synth_state_dict(pack.model_spec(cfg), 83)


@pytest.mark.parametrize("name,odim,ytol", MODELS, ids=[m[0] for m in MODELS])
def test_every_length_without_a_cache(name, odim, ytol):
    cfg, sd = _weights(name, odim)
    a = build(cfg, sd).set_option("stream", 0)
    b = build(cfg, sd).set_option("g16", 0).set_option("stream", 0)
    for T in range(1, 113):
        x = synth.synth_feats(B, T, cfg["input_dim"], seed=2000 + T)
        ya, ca = run(a, x)
        yb, cb = run(b, x)
        ec, ey = max_abs(ca, cb), max_abs(ya, yb)
        assert ec <= 3e-6 * max(1.0, float(np.abs(cb).max())), (name, T, ec)
        assert ey <= ytol, (name, T, ey)


@pytest.mark.parametrize("name,odim,ytol", MODELS, ids=[m[0] for m in MODELS])
def test_every_length_with_an_incoming_cache(name, odim, ytol):
    cfg, sd = _weights(name, odim)
    a = build(cfg, sd)
    b = build(cfg, sd).set_option("g16", 3)
    x0 = synth.synth_feats(B, 98, cfg["input_dim"], seed=3000)
    _, c0a = run(a, x0)                                       # each model continues the cache its own first call returned
    _, c0b = run(b, x0)
    for T in range(17, 113):
        x = synth.synth_feats(B, T, cfg["input_dim"], seed=3000 + T)
        ya, ca = run(a, x, c0a)
        yb, cb = run(b, x, c0b)
        assert np.array_equal(ca, cb), (name, T, max_abs(ca, cb))
        ey = max_abs(ya, yb)
        assert ey <= 5e-7, (name, T, ey)
