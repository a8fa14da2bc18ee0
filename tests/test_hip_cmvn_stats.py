"""GPU: the global CMVN statistics (wekws_amd.cmvn.CmvnStats -> wekws_hip_cmvn_stats_*) against the exact oracle at the derived
bar of tests/cmvn_stats_ref.py (N 2^-53 sum|term| per bin), on the smallest shapes where the kernels can go wrong: every way a
width meets the lanes (1, 40, 80, the odd 83, 400 and 1030 past one pass), frames around one and two tiles, lengths absent, full,
mixed with empty rows, and all empty.  Beside it torch's float32 sum as the control that the bar is no formality, accumulation over
calls, reset, reproducibility, poisoned padding, non-finite features, bad lengths, an MFMA tenant on a second stream, and the
command-line tool on wavs written here."""
import json
import math
import wave

import numpy as np
import pytest
import torch

from tests import cmvn_stats_ref as ref
from tests.test_hip_tenants import tenant  # noqa: F401  (the MFMA tenants of the second stream)

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def dev_lengths(lengths):
    return None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")


def run(x, lengths, on_device=False):
    from wekws_amd.cmvn import CmvnStats
    st = CmvnStats(x.shape[2])
    st.update(dev(x), dev_lengths(lengths) if on_device else lengths)
    return st.result()


def check(result, want, what):
    um, uv, n_ok, cls = ref.inside(result, want)
    print(what, "units", um, uv, "frames", result["frame_num"])
    assert n_ok, (what, result["frame_num"], want["frame_num"])
    assert cls, (what, "non-finite classes")
    assert um <= 1.0 and uv <= 1.0, (what, um, uv)


@pytest.fixture(scope="module")
def matrix():
    """[(name, x, lengths, oracle)] of every device case, computed once"""
    out = []
    for i, (name, B, T, D, kind) in enumerate(ref.gpu_cases()):
        x = ref.feats_of(B, T, D, seed=100 + i)
        lengths = ref.lengths_of(kind, B, T, seed=100 + i)
        out.append((name, kind, x, lengths, ref.oracle(ref.valid_rows(x, lengths))))
    return out


def test_every_case_is_inside_the_bar(matrix):
    assert len(matrix) >= 30
    for i, (name, kind, x, lengths, want) in enumerate(matrix):
        got = run(x, lengths, on_device=bool(i & 1))                     # host lengths and device lengths take turns
        check(got, want, name)
        if kind == "zero":
            assert got["frame_num"] == 0 and not any(got["mean_stat"]) and not any(got["var_stat"]), name


def test_more_than_64_tiles_fold_in_two_stages():
    """Up to 64 tiles are folded by one launch, more in segments of 64 first: exactly 64 tiles, 65, 129 (a last segment of one
    tile) and 1025 (17 segments; the oracle on a few of its bins, the first and the last among them)."""
    import ctypes
    from wekws_amd import _capi
    out = (ctypes.c_int64 * 3)()
    for D, B, T, kind, tiles, bins in ((1030, 64, 7, "none", 64, None), (1030, 5, 91, "mixed", 65, None), (400, 43, 60, "full", 129, None),
                                       (83, 1025, 98, "mixed", 1025, [0, 1, 41, 82])):
        assert _capi.load().wekws_hip_cmvn_stats_plan(B, T, D, out) == 0 and out[1] == tiles, (D, B, T, list(out))
        x = ref.feats_of(B, T, D, seed=D + B)
        lengths = ref.lengths_of(kind, B, T, seed=D)
        got = run(x, lengths, on_device=True)
        frames = ref.valid_rows(x, lengths)
        if bins is not None:
            frames = frames[:, bins]
            got = {"mean_stat": [got["mean_stat"][c] for c in bins], "var_stat": [got["var_stat"][c] for c in bins], "frame_num": got["frame_num"]}
        check(got, ref.oracle(frames), f"{tiles} tiles")


def test_every_frame_finds_its_row():
    """The kernel numbers the frames row by row and finds frame f's row as f / T by a multiplication (cmvn_stats_plan.h): every
    T from 1 to 70, and some around powers of two, with lengths that cut every row differently and three bins (85 frames side by
    side), so a frame taken for the wrong row's shows in the sums."""
    from wekws_amd.cmvn import CmvnStats
    st = CmvnStats(3)
    for T in list(range(1, 71)) + [127, 128, 129, 1023, 1025, 4097, 65535, 65537]:
        B = 7 if T < 5000 else 3
        x = ref.feats_of(B, T, 3, seed=T)
        lengths = [(b * 2654435761 + T) % (T + 1) for b in range(B)]
        st.reset()
        st.update(dev(x), dev_lengths(lengths))
        got, want = st.result(), ref.float64_accumulation(x, lengths)
        assert got["frame_num"] == want["frame_num"], T
        # against numpy's double sums: both are within the bar of the exact sums, so within twice the bar of each other
        frames = ref.valid_rows(x, lengths)
        for key, terms in (("mean_stat", np.abs(frames).sum(axis=0)), ("var_stat", (frames * frames).sum(axis=0))):
            slack = 2 * max(want["frame_num"], 1) * ref.U * terms
            assert (np.abs(np.asarray(got[key]) - np.asarray(want[key])) <= slack).all(), (T, key)


def test_torch_float32_sum_misses_the_same_bar(matrix):
    """The control: feats.sum((0, 1)) in float32 on the device, on the cases where every frame counts and there are at least 16
    of them (tests/test_cmvn_stats_ref.py shows no float32 can meet the bar there)."""
    seen = 0
    for name, kind, x, lengths, want in matrix:
        B, T, _ = x.shape
        if not ref.is_negative_control(B, T, kind):
            continue
        f = dev(x)
        got = {"mean_stat": f.sum((0, 1)).cpu().numpy(), "var_stat": (f * f).sum((0, 1)).cpu().numpy(), "frame_num": B * T}
        um, uv, n_ok, _ = ref.inside(got, want)
        print(name, "torch float32 units", um, uv)
        assert um > 1.0 and uv > 1.0 and n_ok, (name, um, uv)
        seen += 1
    assert seen >= 8


def test_two_updates_then_read_and_reset():
    from wekws_amd.cmvn import CmvnStats
    D = 83
    tile = ref.tile_frames(D)
    xa, la = ref.feats_of(3, tile + 1, D, seed=7), [tile + 1, 5, 0]
    xb, lb = ref.feats_of(5, 2 * tile + 1, D, seed=8), None
    st = CmvnStats(D)
    st.update(dev(xa), la).update(dev(xb), lb)
    both = ref.oracle(np.concatenate([ref.valid_rows(xa, la), ref.valid_rows(xb, lb)]))
    check(st.result(), both, "two updates")                              # N is the total
    assert both["frame_num"] == tile + 6 + 5 * (2 * tile + 1)
    st.reset()
    zero = st.result()
    assert zero["frame_num"] == 0 and not any(zero["mean_stat"]) and not any(zero["var_stat"])
    st.update(dev(xb), lb)
    check(st.result(), ref.oracle(ref.valid_rows(xb, lb)), "after reset")
    assert st.result() == run(xb, lb)                                    # and the bits of a fresh handle


def test_the_same_call_twice_gives_the_same_bits():
    from wekws_amd.cmvn import CmvnStats
    x, lengths = ref.feats_of(5, 203, 80, seed=11), [203, 0, 17, 202, 101]
    f, n = dev(x), dev_lengths(lengths)
    a = run(x, lengths)
    st = CmvnStats(80)
    for _ in range(3):
        st.reset()
        st.update(f, n)
        assert st.result() == a
    # the scratch of a larger call before it changes nothing
    st.reset()
    st.update(dev(ref.feats_of(5, 900, 80, seed=12)))
    st.reset()
    st.update(f, n)
    assert st.result() == a


def test_poisoned_padding_changes_nothing():
    for D, T in ((83, ref.tile_frames(83) + 1), (1030, 2 * ref.tile_frames(1030) + 1), (1, 300)):
        x = ref.feats_of(5, T, D, seed=21)
        lengths = [T - 1, 0, T, T // 2, 1]
        clean = run(x, lengths)
        dirty = x.copy()
        for b, n in enumerate(lengths):
            dirty[b, n:] = (math.nan, math.inf, -math.inf, 3.0e38, math.nan)[b]
        assert run(dirty, lengths) == clean, (D, T)
        assert run(dirty, lengths, on_device=True) == clean, (D, T)
        check(clean, ref.oracle(ref.valid_rows(x, lengths)), f"padding {D}")


def test_non_finite_features_propagate_per_bin():
    D = 83
    T = ref.tile_frames(D) + 1
    x = ref.feats_of(3, T, D, seed=31)
    lengths = [T, T - 2, 3]
    x[0, 5, 2] = math.nan
    x[1, 0, 7] = math.inf
    x[2, 2, 11] = -math.inf
    x[0, T - 1, 13], x[1, T - 3, 13] = math.inf, -math.inf               # both: NaN in mean_stat, +Inf in var_stat
    x[1, T - 1, 17] = math.nan                                           # in the padding: must not show
    want = ref.oracle(ref.valid_rows(x, lengths))
    got = run(x, lengths)
    assert math.isnan(got["mean_stat"][2]) and math.isnan(got["var_stat"][2])
    assert got["mean_stat"][7] == math.inf and got["var_stat"][7] == math.inf
    assert got["mean_stat"][11] == -math.inf and got["var_stat"][11] == math.inf
    assert math.isnan(got["mean_stat"][13]) and got["var_stat"][13] == math.inf
    assert math.isfinite(got["mean_stat"][17])
    check(got, want, "non-finite")                                       # the classes per bin, every other bin inside the bar
    assert np.isfinite(want["mean_stat"]).sum() == D - 4


def test_large_finite_sums_do_not_overflow():
    """the one deviation: 8 frames of 3e38 overflow float32 (the reference's sum is inf), the double sums hold them"""
    x = np.full((2, 4, 3), 3.0e38, dtype=np.float32)
    got = run(x, None)
    check(got, ref.oracle(ref.valid_rows(x, None)), "3e38")
    assert all(math.isfinite(v) for v in got["mean_stat"] + got["var_stat"])
    assert not math.isfinite(ref.reference_float32(x, None)["mean_stat"][0])


def test_bad_lengths_on_the_device_are_skipped_and_counted():
    from wekws_amd.cmvn import CmvnStats
    D = 40
    T = ref.tile_frames(D) + 1
    x = ref.feats_of(5, T, D, seed=41)
    st = CmvnStats(D)
    st.update(dev(x), dev_lengths([T, -1, 7, T + 1, 0]))
    mean, var, n, bad = st.read()
    assert bad == 2 and n == T + 7
    want = ref.oracle(ref.valid_rows(x, [T, 0, 7, 0, 0]))
    check({"mean_stat": mean, "var_stat": var, "frame_num": n}, want, "bad rows skipped")
    with pytest.raises(ValueError, match="2 rows"):
        st.result()
    with pytest.raises(ValueError):
        st.save("/nonexistent/never/written")
    st.reset()
    assert st.result()["frame_num"] == 0                                  # reset clears the count of bad rows too
    st.update(dev(x), torch.tensor([T, 2 ** 40, 7, -2 ** 40, 0], dtype=torch.int64, device="cuda"))        # int64 that would wrap
    assert st.read()[2:] == (T + 7, 2)


def test_bad_host_arguments_raise_before_any_launch():
    from wekws_amd.cmvn import CmvnStats
    D, T = 40, 9
    x = dev(ref.feats_of(3, T, D, seed=51))
    st = CmvnStats(D)
    for lengths in ([T, -1, 3], [T, T + 1, 3], [T, 3], np.asarray([1, 2, 10]), torch.tensor([0, 0, -5])):
        with pytest.raises(ValueError):
            st.update(x, lengths)
    with pytest.raises(ValueError, match="bins"):
        st.update(dev(ref.feats_of(3, T, D + 1, seed=52)))
    for bad in (x.cpu(), x.double(), x[0], x.to(torch.float16)):
        with pytest.raises(ValueError):
            st.update(bad)
    with pytest.raises(ValueError):
        CmvnStats(0)
    with pytest.raises(ValueError):
        CmvnStats(4097)
    assert st.read()[2:] == (0, 0) and not st.read()[0].any()            # nothing ran
    st.update(x[:0]).update(x[:, :0])                                    # empty batches are fine and add nothing
    assert st.result()["frame_num"] == 0
    st.update(x[:, 1:4])                                                 # a view: made contiguous, not misread
    check(st.result(), ref.oracle(ref.valid_rows(x.cpu().numpy()[:, 1:4], None)), "view")


def test_mean_istd_is_load_cmvn_of_the_saved_file(tmp_path):
    from wekws_amd.cmvn import CmvnStats, merge_cmvn_stats
    from wekws_amd.utils.cmvn import load_cmvn
    x, lengths = ref.feats_of(5, 120, 80, seed=61), [120, 64, 0, 119, 1]
    st = CmvnStats(80)
    st.update(dev(x), lengths)
    path = str(tmp_path / "global_cmvn")
    st.save(path)
    assert json.load(open(path)) == st.result()
    assert st.mean_istd().tobytes() == load_cmvn(path).tobytes()
    # row shards on handles of their own, merged on the host
    shards = [run(x[b:b + 1], lengths[b:b + 1]) for b in range(5)]
    check(merge_cmvn_stats(shards), ref.oracle(ref.valid_rows(x, lengths)), "merged shards")


def test_cmvn_stats_beside_an_mfma_tenant(tenant):  # noqa: F811
    """update on one stream, an MFMA-heavy forward on another: bit-identical to the solo run"""
    from wekws_amd.cmvn import CmvnStats
    rng = np.random.default_rng(71)
    cases = []
    for B, T, D in ((1024, 98, 80), (64, 98, 83), (16, 40, 1030)):
        f = dev((10.0 + 4.0 * rng.standard_normal((B, T, D))).astype(np.float32))
        n = torch.from_numpy(rng.integers(0, T + 1, size=B).astype(np.int32)).cuda()
        cases.append((CmvnStats(D), f, n))

    def work():
        out = []
        for st, f, n in cases:
            st.reset()
            st.update(f, n).update(f)
            out.append(st)
        return out

    solo = [st.result() for st in work()]
    tm, tx = tenant
    torch.cuda.synchronize()
    s_a, s_b = torch.cuda.Stream(), torch.cuda.Stream()
    for rnd in range(4):
        with torch.cuda.stream(s_b):
            for _ in range(8):
                tm(tx)
        with torch.cuda.stream(s_a):
            got = [st.result() for st in work()]
        torch.cuda.synchronize()
        assert got == solo, rnd


def _write_wav(path, pcm, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(pcm, dtype="<i2").tobytes())


@pytest.mark.parametrize("feats_type", ["fbank", "mfcc"])
def test_the_command_line_tool(tmp_path, feats_type):
    from wekws_amd.bin import compute_cmvn_stats as tool
    from wekws_amd.cmvn import CmvnStats
    from wekws_amd.frontend import Fbank, Resample
    rng = np.random.default_rng(81)
    wavs = {"a": (16000, 16000), "b": (16000, 9000), "c": (8000, 7000)}          # name -> (rate, samples); c is resampled
    for name, (rate, n) in wavs.items():
        _write_wav(tmp_path / f"{name}.wav", np.round(rng.standard_normal(n) * 3000.0).clip(-32768, 32767), rate)
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(f"utt_{k} {tmp_path / (k + '.wav')}\n" for k in wavs) + f"utt_seg {tmp_path / 'a.wav'},0.25,0.8125\n")
    conf = tmp_path / "train.yaml"
    conf.write_text(f"dataset_conf:\n  feats_type: {feats_type}\n  {feats_type}_conf:\n    num_mel_bins: 40\n"
                    "  resample_conf:\n    resample_rate: 16000\n")
    out = tmp_path / "global_cmvn"
    tool.main(["--train_config", str(conf), "--in_scp", str(scp), "--out_cmvn", str(out), "--num_workers", "4"])
    got = json.load(open(out))
    fb = Fbank(40, window="povey")
    samples = [16000, 9000, Resample(8000).num_samples(7000), int(0.8125 * 16000) - int(0.25 * 16000)]
    assert got["frame_num"] == sum(fb.num_frames(n) for n in samples) > 0
    assert len(got["mean_stat"]) == len(got["var_stat"]) == 40
    # the same feature batches into a handle of the test's own: the same bits; and their exact sums: inside the bar
    st, rows = CmvnStats(40), []
    for feats, frames in tool.feature_batches(tool.read_scp(str(scp)), feats_type, 40, 16000):
        st.update(feats, frames)
        host = feats.cpu().numpy()
        rows += [host[b, :n] for b, n in enumerate(frames)]
    assert st.result() == got
    check(got, ref.oracle(np.concatenate(rows).astype(np.float64)), f"tool {feats_type}")


def test_the_tool_refuses_other_sample_formats(tmp_path):
    from wekws_amd.bin import compute_cmvn_stats as tool
    path = tmp_path / "u8.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(1)
        w.setframerate(16000)
        w.writeframes(bytes(range(200)))
    with pytest.raises(SystemExit, match="16-bit"):
        tool.read_wav(str(path))
