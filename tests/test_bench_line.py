"""CPU: the shape of bench.py's stdout -- the contract line is LAST, compact, the only line that starts with '{'; the verbose
records go to the side file and to `extras <key> = ...` lines.  (Round 5's single 22.5 KB line could not be parsed by the
driver; the GPU run of the same check is tests/test_hip_bench.py.)"""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _line(**more):
    roof = bench.mfma_roofline("ds_tcn_h256", 1024, 0.2, "f16x3")
    roof.update(kernel="ds256_g16_kernel<7,true,true,false>", traffic=207_100_000, traffic_unit="x" * 900,
                traffic_source="profiles/r06_x.txt", kernel_avg_ms_rocprof=0.197)
    out = {"metric": "m", "value": 5.0e6, "unit": "utts/s", "n_gpus": 1, "steps": 20, "warmup": 5, "ms_per_step": 0.2,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "w"}, "roofline": bench.compact_roofline(roof),
           "cpu_baseline": {"value": 1.0, "unit": "utts/s", "cores": 1, "kind": "port", "sample": "s"}}
    out.update(more)
    return out, roof


def test_emit_puts_the_compact_line_last(tmp_path):
    out, roof = _line()
    extra = {"roofline_verbose": roof, "big": {"rows": ["y" * 100] * 300}}          # ~30 KB of extras
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.emit(out, extra, str(tmp_path / "x" / "extras.json"))
    lines = buf.getvalue().splitlines()
    assert lines[-1].startswith('{"metric"') and len(lines[-1]) < bench.MAX_LINE_BYTES
    assert sum(ln.startswith("{") for ln in lines) == 1
    d = json.loads(lines[-1])
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms", "algorithmic_bytes_per_launch"):
        assert k in d["roofline"], k
    assert "traffic_unit" not in d["roofline"]
    side = json.load(open(tmp_path / "x" / "extras.json"))
    assert side["extras"]["big"]["rows"][0] == "y" * 100 and side["contract_line"]["value"] == d["value"]
    tail = buf.getvalue().encode()[-8192:].decode()
    assert json.loads(tail[tail.rindex('{"metric"'):]) == d                          # survives the driver's 8 KB tail


def test_emit_refuses_a_line_that_outgrew_the_tail(tmp_path):
    out, _ = _line(bloat="z" * 7000)
    with pytest.raises(AssertionError):
        with redirect_stdout(io.StringIO()):
            bench.emit(out, {}, str(tmp_path / "e.json"))


def test_dump_outputs_keeps_small_arrays_and_samples_large_ones(tmp_path):
    """--dump-outputs: arrays within their share of the 64 MB are written whole; a larger one as a seeded sample of its rows,
    the same rows every run, with the row numbers beside it (float64)."""
    import numpy as np
    import torch
    y = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    big = torch.randn(80, 1 << 17)                                   # 40 MB > a 32 MB share
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"posteriors": y, "cache": big}, 0, 1)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["cache_sample.npy", "cache_sample_index.npy", "posteriors.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BYTES
    assert np.array_equal(np.load(tmp_path / "a" / "posteriors.npy"), y.numpy())
    idx = np.load(tmp_path / "a" / "cache_sample_index.npy")
    share = bench.DUMP_BYTES // 2                                    # two arrays; the sample pays for its index and headers
    assert len(idx) == (share - 2 * bench.NPY_HEADER_BYTES) // (big[0].numel() * 4 + 8) == 63
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "cache_sample.npy"), big.numpy()[idx.astype(np.int64)])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    bench.dump_outputs(str(tmp_path / "r"), {"posteriors": y}, 1, 2)
    assert os.listdir(tmp_path / "r") == ["posteriors_rank1.npy"]
    # one row larger than the share (3 rows of 40 MB): single elements of the flattened array, still within the cap
    wide = torch.randn(3, 10 << 20)
    bench.dump_outputs(str(tmp_path / "w"), {"posteriors": y, "cache": wide}, 0, 1)
    assert sum(os.path.getsize(tmp_path / "w" / f) for f in os.listdir(tmp_path / "w")) <= bench.DUMP_BYTES
    idx = np.load(tmp_path / "w" / "cache_sample_index.npy").astype(np.int64)
    assert len(idx) == (share - 2 * bench.NPY_HEADER_BYTES) // 12
    assert np.array_equal(np.load(tmp_path / "w" / "cache_sample.npy"), wide.numpy().reshape(-1)[idx])


def test_steps_below_one_are_refused():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


def test_full_option_and_the_plain_line():
    """A plain run measures the headline alone; everything else is behind --full, which every caller that needs it passes."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--full" in r.stdout
    buf = io.StringIO()
    out, _ = _line()
    with redirect_stdout(buf):
        bench.print_line(out)
    assert buf.getvalue().splitlines() == [json.dumps(out)]
