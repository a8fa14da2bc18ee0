"""GPU: the fused utterance boundary of the persistent ds256_g16 kernel (wekws_amd/csrc/ds256_g16.hip.h).

A persistent workgroup walks over utterances b, b + grid, ...; every utterance after the first of a walk is staged under the
classifier of the one before (its features taken from LDS, its maximum published, its operand planes written, its input layer
multiplied) and enters the loop at the residual blocks.  The first utterance of a walk, the one behind an utterance that left the
fast path for non-finite input, and every one-pass launch (option g16 = 2: one utterance per workgroup) take the cold prologue.

The yardstick is therefore the SAME kernel run one utterance per workgroup: it executes the same instructions on the same data, so
the persistent run must equal it bit for bit -- posteriors and returned cache, every row of every batch."""
import numpy as np
import pytest
import torch

from oracle import kws_oracle
from tests.helpers import POSTERIOR_TOL, max_abs, tol_for
from tests.test_hip_parity import build, run
from wekws_amd import pack
from wekws_amd.utils import synth

pytestmark = pytest.mark.gpu

T_HEAD = 98


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def weights():
    cfg = dict(synth.MODEL_CONFIGS["ds_tcn_h256"])
    return cfg, synth.synth_state_dict(pack.model_spec(cfg), 1234)


@pytest.fixture(scope="module")
def pair(weights):
    """(persistent, one utterance per workgroup) models of one precision, built once."""
    cfg, sd = weights
    made = {}

    def get(precision="default"):
        if precision not in made:
            made[precision] = (build(cfg, sd).set_precision(precision), build(cfg, sd).set_precision(precision).set_option("g16", 2))
        return made[precision]
    return get


def posteriors(model, x):
    y = model.posteriors(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.fixture(scope="module")
def walk_batch(weights, cus):
    """The largest batch of the walk-length cases and its oracle, computed once; the smaller batches are its leading rows."""
    cfg, sd = weights
    x = synth.synth_feats(3 * cus + 5, T_HEAD, cfg["input_dim"], seed=31)
    ry, rc = kws_oracle.forward(cfg, sd, x, None)
    return x, ry, rc


@pytest.mark.parametrize("kind", ["cus+1", "2cus", "2cus+1", "3cus+5"])
def test_walk_lengths(kind, pair, walk_batch, cus):
    """Walks of 1 and 2, exactly 2, 2 and 3, and 3 and 4 utterances; forward (with cache) and posteriors (no cache out); and the oracle."""
    B = {"cus+1": cus + 1, "2cus": 2 * cus, "2cus+1": 2 * cus + 1, "3cus+5": 3 * cus + 5}[kind]
    xa, rya, rca = walk_batch
    x, ry, rc = xa[:B], rya[:B], rca[:B]
    pers, one = pair()
    y, c = run(pers, x)
    y1, c1 = run(one, x)
    assert np.array_equal(y, y1), (B, max_abs(y, y1))
    assert np.array_equal(c, c1), (B, max_abs(c, c1))
    yp, yp1 = posteriors(pers, x), posteriors(one, x)
    assert np.array_equal(yp, yp1) and np.array_equal(yp, y), B
    assert y.shape == ry.shape and max_abs(y, ry) <= POSTERIOR_TOL, (B, max_abs(y, ry))
    assert max_abs(c, rc) <= tol_for(rc), (B, max_abs(c, rc))


@pytest.mark.parametrize("T", [5, 33, 97, 100, 112])
def test_every_tile_count_and_ragged_ends(T, pair, weights, cus):
    """One tile (the partial sums end exactly where the planes end), the middle tile counts, and seven tiles with a last lane that
    is not full, over-full and full."""
    cfg, _ = weights
    pers, one = pair()
    x = synth.synth_feats(2 * cus + 3, T, cfg["input_dim"], seed=200 + T)
    y, c = run(pers, x)
    y1, c1 = run(one, x)
    assert np.array_equal(y, y1), (T, max_abs(y, y1))
    assert np.array_equal(c, c1), (T, max_abs(c, c1))
    assert np.array_equal(posteriors(pers, x), posteriors(one, x)), T


def test_one_product_precision(pair, weights, cus):
    """SPLIT = false: precision "f16"."""
    cfg, _ = weights
    pers, one = pair("f16")
    x = synth.synth_feats(2 * cus + 3, T_HEAD, cfg["input_dim"], seed=41)
    y, c = run(pers, x)
    y1, c1 = run(one, x)
    assert np.array_equal(y, y1) and np.array_equal(c, c1), (max_abs(y, y1), max_abs(c, c1))
    assert np.array_equal(posteriors(pers, x), posteriors(one, x))


def test_context_variant(pair, weights, cus):
    """A second chunk with the carried cache (80 frames): the context variant keeps the cold sequence for every utterance of a walk;
    persistent == one utterance per workgroup bit for bit, and the cache == ds256_w16's (option g16 = 3) bit for bit."""
    cfg, sd = weights
    pers, one = pair()
    w16 = build(cfg, sd).set_option("g16", 3)
    B = 2 * cus + 3
    x = synth.synth_feats(B, 40 + 80, cfg["input_dim"], seed=51)
    _, c0 = run(pers, x[:, :40])
    x2 = np.ascontiguousarray(x[:, 40:])
    y, c = run(pers, x2, c0)
    y1, c1 = run(one, x2, c0)
    assert np.array_equal(y, y1) and np.array_equal(c, c1), (max_abs(y, y1), max_abs(c, c1))
    yw, cw = run(w16, x2, c0)
    assert np.array_equal(c, cw), max_abs(c, cw)
    assert max_abs(y, yw) <= 5e-7, max_abs(y, yw)


# ---- non-finite rows inside a walk: B = 3 cus + 2; workgroup g walks rows g, g + cus, g + 2 cus (g = 0, 1: and g + 3 cus)
POISON_PATTERNS = {
    "first": (1, (0,)), "middle": (1, (1,)), "last": (1, (2,)), "first+middle": (1, (0, 1)), "middle+last": (1, (1, 2)),
    "all-three": (1, (0, 1, 2)),
    # workgroup 5 walks exactly three rows: here "last" is the walk's last utterance
    "first/3": (5, (0,)), "middle/3": (5, (1,)), "last/3": (5, (2,)), "first+middle/3": (5, (0, 1)), "middle+last/3": (5, (1, 2)),
    "all-three/3": (5, (0, 1, 2)),
    # a walk of four: the row whose successor is the walk's last row; and that last row itself
    "third-of-four": (0, (2,)), "second+third-of-four": (0, (1, 2)), "fourth-of-four": (0, (3,)),
}


@pytest.fixture(scope="module")
def clean_runs(pair, weights, cus):
    cfg, _ = weights
    x = synth.synth_feats(3 * cus + 2, T_HEAD, cfg["input_dim"], seed=61)
    got = {}

    def get(precision):
        if precision not in got:
            got[precision] = run(pair(precision)[0], x)
        return (x,) + got[precision]
    return get


@pytest.mark.parametrize("precision", ["default", "f32"])
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("pattern", list(POISON_PATTERNS))
def test_nonfinite_rows_inside_a_walk(pattern, value, precision, pair, clean_runs, cus):
    """A poisoned row leaves the fast path -- noticed in the cold prologue (first of a walk, or behind another bad row) or in phase 2 of
    the boundary -- and the walk goes on cold behind it.  Equal to the one-pass run of the same input (NaN == NaN), and every clean
    row bit-identical to the run of the clean batch.  "f32" runs ds256_g32, which shares the helpers."""
    g, steps = POISON_PATTERNS[pattern]
    x0, y0, c0 = clean_runs(precision)
    rows = [g + s * cus for s in steps]
    assert max(rows) < len(x0)
    x = x0.copy()
    for i, r in enumerate(rows):
        x[r, (7 * r + 3 * i) % T_HEAD, (r + i) % x.shape[2]] = value
    pers, one = pair(precision)
    y, c = run(pers, x)
    y1, c1 = run(one, x)
    assert np.array_equal(y, y1, equal_nan=True), pattern
    assert np.array_equal(c, c1, equal_nan=True), pattern
    clean = np.ones(len(x), bool)
    clean[rows] = False
    assert np.array_equal(y[clean], y0[clean]) and np.array_equal(c[clean], c0[clean]), pattern


def test_two_launches_back_to_back(pair, weights, cus):
    """Nothing survives a launch in LDS-side state: the second launch of a model equals a fresh model's."""
    cfg, sd = weights
    pers, _ = pair()
    xa = synth.synth_feats(2 * cus + 3, T_HEAD, cfg["input_dim"], seed=71)
    xb = synth.synth_feats(cus + 7, T_HEAD, cfg["input_dim"], seed=72)
    run(pers, xa)
    y, c = run(pers, xb)
    yf, cf = run(build(cfg, sd), xb)
    assert np.array_equal(y, yf) and np.array_equal(c, cf), (max_abs(y, yf), max_abs(c, cf))
