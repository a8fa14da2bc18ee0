"""CPU: the yardstick of the dithered front end (tests/dither_ref.py) checked on its own -- the generator against published
vectors, the distribution and independence of the oracle's field, and the calibration of the two bars the GPU test
(tests/test_hip_dither.py) holds the kernels to.  The distribution is asserted HERE, on the oracle alone, so the GPU test, which
compares the kernels with the oracle element by element, cannot hide behind a statistical bar."""
import numpy as np
import pytest

from tests import dither_ref as dr
from tests.helpers import K_FBANK, pow2_at_or_above

N = 2 ** 20
FIELD = (8, 328, 400)                            # rows x frames x samples: 1,049,600 values, truncated to N


def test_philox_known_answers():
    """Counter / key -> output, equal to Random123's published vectors for philox4x32_10."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        assert " ".join(f"{int(v):08x}" for v in dr.philox4x32_10(counter, key)) == want


def test_uniforms_are_float32_values_strictly_inside_the_unit_interval():
    words = np.array([0, 1, 0x1FF, 0x200, 0x7FFFFFFF, 0x80000000, 0xFFFFFE00, 0xFFFFFFFF], np.uint32)
    u = dr.uniform(words)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u) and u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    assert np.sqrt(-2.0 * np.log(u.min())) >= 5.5


def test_sample_mapping_uses_every_word_of_two_blocks_per_lane():
    """Samples 0 .. 511 of a frame: 128 blocks x 4 words, each (block, word) exactly once; the four sample pairs l + 64 m of an fbank
    lane l sit in the blocks l and l + 64."""
    i = np.arange(512)
    blk, w = dr.sample_map(i)
    word = w + (i & 1)
    assert len({(int(b), int(x)) for b, x in zip(blk, word)}) == 512 and blk.max() == 127 and word.max() == 3
    for lane in (0, 17, 63):
        pairs = lane + 64 * np.arange(4)
        b, _ = dr.sample_map(2 * pairs)
        assert b.tolist() == [lane, lane, lane + 64, lane + 64]


@pytest.fixture(scope="module")
def field():
    return dr.normal_field(dr.SEED, 0, *FIELD)


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_distribution_of_the_oracle_field(field):
    from scipy.special import ndtr
    z = field.ravel()[:N]
    assert abs(z.mean()) <= 5.0 / np.sqrt(N)
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / N)
    cdf = ndtr(np.sort(z))
    k = np.arange(N)
    ks = max(float(np.max((k + 1) / N - cdf)), float(np.max(cdf - k / N)))
    assert ks <= 2.5 / np.sqrt(N), ks                        # (a correct generator exceeds it with probability about 7e-6)
    assert np.abs(z).max() <= np.sqrt(48.0 * np.log(2.0))


def test_lag_correlations_of_the_oracle_field(field):
    bar = 5.0 / np.sqrt(N)
    assert abs(_corr(field[:, :, :-1], field[:, :, 1:])) <= bar                  # sample i and i + 1 of a frame
    assert abs(_corr(field[:, :, 0::2], field[:, :, 1::2])) <= bar               # the cosine and the sine of one pair
    assert abs(_corr(field[:, :-1, 160:], field[:, 1:, :240])) <= bar            # one waveform sample seen by two overlapping frames
    assert abs(_corr(field[:-1], field[1:])) <= bar                              # the same (frame, sample) of two rows
    other = dr.normal_field(dr.SEED + 1, 0, *FIELD)
    assert abs(_corr(field, other)) <= bar                                       # ... of two seeds


def test_no_two_blocks_are_equal():
    """2^16 blocks across rows, frames and seeds: all different."""
    blocks = []
    for seed in (dr.SEED, dr.SEED + 1):
        c0 = np.arange(128, dtype=np.uint64)[None, None, :]
        c1 = np.arange(64, dtype=np.uint64)[None, :, None]
        c2 = np.arange(4, dtype=np.uint64)[:, None, None]
        w = np.stack(dr.philox4x32_10((c0, c1, c2, np.zeros_like(c2)), (seed & 0xFFFFFFFF, seed >> 32)), axis=-1)
        blocks.append(w.reshape(-1, 4))
    blocks = np.concatenate(blocks)
    assert blocks.shape == (2 ** 16, 4) and np.unique(blocks, axis=0).shape[0] == 2 ** 16


def test_k_noise_z_is_twice_the_float32_evaluation(field):
    """K_NOISE_Z: the smallest power of two at or above twice the worst error of the numpy float32 evaluation of the same formulas,
    over the GPU test's fields -- and over the distribution test's 2^20 values, which give the same bar."""
    worst = 0.0
    for B, nf, fl in dr.NOISE_FIELDS:
        for row in dr.NOISE_FIRST_ROWS:
            for seed in (dr.SEED, dr.SEED_HI):
                worst = max(worst, float(dr.noise_units(dr.normal_field_f32(seed, row, B, nf, fl), dr.normal_field(seed, row, B, nf, fl)).max()))
    big = float(dr.noise_units(dr.normal_field_f32(dr.SEED, 0, *FIELD), field).max())
    print(f"float32 noise field: {worst:.2f} (the GPU test's fields), {big:.2f} (8 x 328 x 400)")
    assert pow2_at_or_above(2.0 * worst) == dr.K_NOISE_Z == pow2_at_or_above(2.0 * big), (worst, big)


def test_bars_follow_the_float32_restatement():
    """The calibration of the feature bar: fbank_f32_exact on float32(x + float32(dither z)) over the GPU test's cases.  Noise and
    silence rows stay within K_FBANK / 2, the project's rule, so they are held to K_FBANK; every full-scale DC row gets the bar the
    same rule gives for it (dither_ref.K_DITHER_DC says why those rows differ on both sides)."""
    worst = {}
    for case in dr.CASES:
        for b, kind in enumerate(dr.KINDS):
            feats, frames = dr.f32_restatement(case, b)
            u = float(dr.frame_units(feats, frames, *dr.case_cfg(case)).max())
            print(f"{case['id']} {kind}: {u:.2f}")
            if kind == "dc":
                assert pow2_at_or_above(2.0 * u) == dr.K_DITHER_DC[case["id"]], (case["id"], u)
            else:
                worst[kind] = max(worst.get(kind, 0.0), u)
    assert max(worst.values()) <= K_FBANK / 2, worst
    assert set(dr.K_DITHER_DC) == {c["id"] for c in dr.CASES}


def test_cases_cover_what_the_kernel_branches_on():
    from tests.fbank_matrix import pair_ok
    ids = {c["id"] for c in dr.CASES}
    assert len(ids) == len(dr.CASES)
    seen = {(c["bins"] > 64, c["dtype"], pair_ok(c["nsamp"], c["shift"], c["flen"], 0, c["dtype"])) for c in dr.CASES if c["flen"] >= 400}
    assert len(seen) == 8                                    # rounds 1 / 2 x float / int16 x pair / per-sample fetch
    assert {(c["flen"], c["shift"]) for c in dr.CASES} == {(400, 160), (512, 160), (65, 33), (400, 400)}
    assert {c["dither"] for c in dr.CASES} == {1.0, 0.25, 37.5}
