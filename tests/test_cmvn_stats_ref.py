"""CPU: the yardstick of the global CMVN statistics holds what it should and lets through what it should not
(tests/cmvn_stats_ref.py), and the host side of wekws_amd/cmvn.py (the file, mean_istd, merge_cmvn_stats)."""
import json
import math

import numpy as np
import pytest

from tests import cmvn_stats_ref as ref
from wekws_amd import cmvn
from wekws_amd.utils.cmvn import load_cmvn


@pytest.fixture(scope="module")
def cases():
    out = {}
    for i, (name, B, T, D, kind) in enumerate(ref.CPU_CASES):
        x = ref.feats_of(B, T, D, seed=i)
        lengths = ref.lengths_of(kind, B, T, seed=i)
        out[name] = (x, lengths, ref.oracle(ref.valid_rows(x, lengths)))
    return out


NAMES = [c[0] for c in ref.CPU_CASES]


@pytest.mark.parametrize("name", NAMES)
def test_a_float64_accumulation_is_inside_the_bar(cases, name):
    x, lengths, want = cases[name]
    um, uv, n_ok, cls = ref.inside(ref.float64_accumulation(x, lengths), want)
    print(name, "float64 units", um, uv)
    assert um <= 1.0 and uv <= 1.0 and n_ok and cls


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_float32_accumulation_misses_the_bar(cases, name):
    x, lengths, want = cases[name]
    um, uv, n_ok, _ = ref.inside(ref.reference_float32(x, lengths), want)
    print(name, "float32 units", um, uv)
    assert um > 1.0 and uv > 1.0 and n_ok


@pytest.mark.parametrize("name", NAMES)
def test_the_saved_file_is_what_load_cmvn_reads(cases, name, tmp_path):
    x, lengths, _ = cases[name]
    stats = ref.float64_accumulation(x, lengths)
    path = str(tmp_path / "global_cmvn")
    cmvn.save_cmvn_stats(stats, path)
    on_disk = json.load(open(path))
    assert sorted(on_disk) == ["frame_num", "mean_stat", "var_stat"] and on_disk == stats       # every double survives the text
    got, want = cmvn.mean_istd(stats), load_cmvn(path)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape == (2, x.shape[2])
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_merged_row_shards_are_inside_the_bar(cases, name):
    x, lengths, want = cases[name]
    shards = [ref.float64_accumulation(x[b:b + 1], None if lengths is None else lengths[b:b + 1]) for b in range(x.shape[0])]
    merged = cmvn.merge_cmvn_stats(shards)
    um, uv, n_ok, cls = ref.inside(merged, want)
    assert um <= 1.0 and uv <= 1.0 and n_ok and cls
    assert all(isinstance(v, float) for v in merged["mean_stat"] + merged["var_stat"]) and isinstance(merged["frame_num"], int)


def test_merge_refuses_what_does_not_fit():
    a = {"mean_stat": [1.0, 2.0], "var_stat": [1.0, 4.0], "frame_num": 1}
    with pytest.raises(ValueError):
        cmvn.merge_cmvn_stats([])
    with pytest.raises(ValueError):
        cmvn.merge_cmvn_stats([a, {"mean_stat": [1.0], "var_stat": [1.0], "frame_num": 1}])
    assert cmvn.merge_cmvn_stats([a, a]) == {"mean_stat": [2.0, 4.0], "var_stat": [2.0, 8.0], "frame_num": 2}


def test_the_oracle_knows_the_non_finite_classes():
    f = np.asarray([[1.0, math.nan, math.inf, -math.inf, math.inf], [2.0, 1.0, 1.0, 1.0, -math.inf]])
    want = ref.oracle(f)
    assert want["mean_stat"][0] == 3.0 and math.isnan(want["mean_stat"][1]) and want["mean_stat"][2] == math.inf
    assert want["mean_stat"][3] == -math.inf and math.isnan(want["mean_stat"][4])
    assert want["var_stat"][0] == 5.0 and math.isnan(want["var_stat"][1]) and list(want["var_stat"][2:]) == [math.inf] * 3
    good = {"mean_stat": [3.0, math.nan, math.inf, -math.inf, math.nan], "var_stat": [5.0, math.nan, math.inf, math.inf, math.inf], "frame_num": 2}
    assert ref.inside(good, want) == (0.0, 0.0, True, True)
    assert not ref.inside(dict(good, mean_stat=[3.0, 0.0, math.inf, -math.inf, math.nan]), want)[3]      # a dropped NaN
    assert ref.inside(dict(good, mean_stat=[math.nan] + good["mean_stat"][1:]), want)[0] == math.inf     # a NaN where a number belongs


def test_the_device_negative_controls_cannot_pass_by_luck():
    """Whatever its order, a float32 sum is a float32: where the float32 nearest to the exact sum is further from it than the
    bar, every float32 sum misses.  On every case the device test holds torch's float32 sum against the bar some bin is such a
    bin, for both statistics."""
    for i, (name, B, T, D, kind) in enumerate(ref.gpu_cases()):
        if not ref.is_negative_control(B, T, kind):
            continue
        want = ref.oracle(ref.valid_rows(ref.feats_of(B, T, D, seed=100 + i), None))
        for key in ("mean_stat", "var_stat"):
            exact = want[key]
            bar = want["abs_" + key.split("_")[0]] * want["frame_num"] * ref.U
            assert (np.abs(exact.astype(np.float32).astype(np.float64) - exact) > bar).any(), (name, key)
