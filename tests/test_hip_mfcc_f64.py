"""GPU: the DCT / lifter kernel and Mfcc against float64, stage by stage, so that the errors of the stages do not mix:
  * dct_lifter(x) against the float64 DCT / lifter of the same x, per element in the unit eps |lifter_k| sum_j |M[j, k] x_j|
    (oracle/kaldi_feats_oracle.py::dct_lifter_scale), at K_DCT (tests/helpers.py);
  * Mfcc(pcm): its fbank stage against fbank_f64 at K_FBANK, its tail against the float64 tail of the kernel's OWN fbank output.
The kernel computes its DCT matrix itself (there is no table to perturb): its negative control is the CPU emulation in
tests/test_fbank_matrix.py::test_k_dct_is_twice_a_float32_evaluation."""
import numpy as np
import pytest
import torch

from oracle import fbank_oracle, kaldi_feats_oracle as kf
from tests.helpers import K_DCT, K_FBANK
from tests.fbank_matrix import DCT_SHAPES, dct_input
from wekws_amd.frontend import Fbank, Mfcc, dct_lifter
from wekws_amd.utils import synth

pytestmark = pytest.mark.gpu


def dct_units(got, x, nc, q):
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - kf.dct_lifter(x, nc, q, dtype=np.float64)) / kf.dct_lifter_scale(x, nc, q)).max())


@pytest.mark.parametrize("shape", DCT_SHAPES, ids=["x".join(map(str, s)) for s in DCT_SHAPES])
def test_dct_lifter_against_float64(shape, error_report):
    rows, nb, nc, q = shape
    x = dct_input(rows, nb)
    got = dct_lifter(torch.from_numpy(x).cuda(), nc, q).cpu().numpy()
    assert got.shape == (rows, nc)
    u = dct_units(got, x, nc, q)
    print(shape, "u =", u)
    key = f"dct_f64/bins{nb}_ceps{nc}_lifter{int(q)}"
    error_report[key] = max(error_report.get(key, 0.0), u)
    assert u <= K_DCT, u


def test_dct_lifter_rows_around_the_grid(error_report):
    """More row tiles than the kernel's grid (a workgroup walks several tiles of 16 rows) with a ragged last tile."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 16 * 4 * cus * 2 + 5
    x = dct_input(rows, 40, seed=1)
    got = dct_lifter(torch.from_numpy(x).cuda(), 13).cpu().numpy()
    u = dct_units(got, x, 13, 22.0)
    error_report["dct_f64/persistent_rows"] = u
    assert u <= K_DCT, u


@pytest.mark.parametrize("ceps,bins", [(80, 80), (13, 40)])
def test_mfcc_stage_by_stage(ceps, bins, error_report):
    pcm = np.concatenate([synth.synth_pcm(2, 16000, seed=9, kind="noise"), synth.synth_pcm(1, 16000, kind="sine"),
                          synth.synth_pcm(1, 16000, kind="ramp"), synth.synth_pcm(1, 16000, kind="silence")])
    t = torch.from_numpy(pcm).cuda()
    m = Mfcc(ceps, bins)
    got = m(t).cpu().numpy()
    logmel = Fbank(bins, window="povey")(t).cpu().numpy()
    assert got.shape == (5, 98, ceps)
    uf = max(float(fbank_oracle.fbank_units(logmel[i], pcm[i], bins, 16000, 400, 160, 1).max()) for i in range(5))
    ud = dct_units(got.reshape(-1, ceps), logmel.reshape(-1, bins), ceps, 22.0)
    print("fbank stage u =", uf, "; tail u =", ud)
    error_report[f"fbank_f64/mfcc{ceps}_{bins}_fbank_stage"] = uf
    error_report[f"dct_f64/mfcc{ceps}_{bins}_tail"] = ud
    assert uf <= K_FBANK and ud <= K_DCT, (uf, ud)
