"""GPU: the dithered fbank / MFCC front end (wekws_hip_fbank_compute_dither[_i16], wekws_hip_dither_noise) against the yardstick of
tests/dither_ref.py: the noise field element by element against the float64 Box-Muller of the same Philox words, the features bin by
bin against the float64 fbank of the dithered frames (each frame a one-frame utterance of oracle/fbank_oracle.py), four negative
controls that a kernel ignoring an argument -- or the parent commit's plain kernel -- cannot pass, and the invariances the counter
based generator promises, bit for bit.  The bars and their calibration: tests/dither_ref.py, tests/test_dither_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import fbank_oracle
from tests import dither_ref as dr
from tests import fbank_matrix as fm
from tests.helpers import CONTROL_MARGIN, K_FBANK
from wekws_amd import _capi
from wekws_amd.frontend import Fbank, Mfcc, dct_lifter, dither_noise
from wekws_amd.utils import synth

pytestmark = pytest.mark.gpu
WINDOWS = ("hamming", "povey")
LOG_FLOOR = float(np.log(np.finfo(np.float32).eps))


def device_pcm(x, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t.to(torch.int16) if dtype == "i16" else t


def make(case, **kw):
    return Fbank(case["bins"], case["sr"], case["flen"], case["shift"], window=WINDOWS[case["window"]], **kw)


def bits(t):
    return t.contiguous().view(torch.int32)


def test_noise_field_against_the_oracle(error_report):
    worst = 0.0
    for B, nf, fl in dr.NOISE_FIELDS:
        for row in dr.NOISE_FIRST_ROWS:
            for seed in (dr.SEED, dr.SEED_HI):
                got = dither_noise(seed, row, B, nf, fl).cpu().numpy()
                assert got.shape == (B, nf, fl)
                u = float(dr.noise_units(got, dr.normal_field(seed, row, B, nf, fl)).max())
                worst = max(worst, u)
                assert u <= dr.K_NOISE_Z, (B, nf, fl, row, hex(seed), u)
    error_report["dither/noise_field_units"] = worst
    print(f"noise field: {worst:.2f} of {dr.K_NOISE_Z}")
    # a field is a pure function of (seed, row id, frame, sample): rows of another call, frames of a longer one
    a = dither_noise(dr.SEED, 5, 4, 7, 400)
    assert torch.equal(bits(dither_noise(dr.SEED, 7, 1, 3, 400)[0]), bits(a[2, :3]))
    assert torch.equal(bits(dither_noise(dr.SEED, 5, 4, 7, 401)[..., :400]), bits(a))
    assert dither_noise(dr.SEED, 0, 0, 7, 400).shape == (0, 7, 400)
    with pytest.raises(_capi.HipLibraryError):
        dither_noise(dr.SEED, 0, 1, 1, 513)


@pytest.mark.parametrize("case", dr.CASES, ids=[c["id"] for c in dr.CASES])
def test_features_against_the_frame_oracle_and_controls(case, error_report):
    x = dr.case_input(case)
    pcm = device_pcm(x, case["dtype"])
    got = make(case, dither=case["dither"], seed=dr.SEED)(pcm, first_row=dr.FIRST_ROW).cpu().numpy()
    plain = make(case)(pcm).cpu().numpy()
    cfg = dr.case_cfg(case)
    fl, shift, d = case["flen"], case["shift"], case["dither"]
    nf = fbank_oracle.num_frames(case["nsamp"], fl, shift)
    assert got.shape == (3, nf, case["bins"]) and np.isfinite(got).all()
    for b, kind in enumerate(dr.KINDS):
        bar = dr.case_bar(case, kind)
        row = dr.FIRST_ROW + b
        frames = dr.dithered_frames(x[b], dr.SEED, row, fl, shift, d)
        u = float(dr.frame_units(got[b], frames, *cfg).max())
        print(f"{case['id']} {kind}: {u:.2f} of {bar}")
        error_report[f"dither/{case['id']}/{kind}"] = u
        assert u <= bar, (case["id"], kind, u, bar)
        # ---- negative controls: each must miss the bar by CONTROL_MARGIN
        z = dr.normal_field(dr.SEED, row, 1, nf, fl)[0]
        controls = {
            "noise_before_framing": dr.dithered_frames(x[b], dr.SEED, row, fl, shift, d, z=np.repeat(z[:, :1], fl, axis=1)),
            "row_off_by_one": dr.dithered_frames(x[b], dr.SEED, row + 1, fl, shift, d),
            "seed_off_by_one": dr.dithered_frames(x[b], dr.SEED + 1, row, fl, shift, d),
        }
        for name, wrong in controls.items():
            uc = float(dr.frame_units(got[b], wrong, *cfg).max())
            assert uc >= CONTROL_MARGIN * bar, (case["id"], kind, name, uc, bar)
        up = float(dr.frame_units(plain[b], frames, *cfg).max())
        assert up >= CONTROL_MARGIN * bar, (case["id"], kind, "plain fbank", up, bar)
    if d == 1.0:                                              # silence: dither 1.0 lifts every bin off the log(FLT_EPSILON) floor
        assert float(plain[1].max()) <= LOG_FLOOR + 1e-6 and float(got[1].min()) > LOG_FLOOR + 1.0, float(got[1].min())


def test_full_device_batch_walks_the_persistent_stride(error_report):
    """B = 160 x 98 frames through the TEST build of the library (the product's own kernel objects plus the launch record): the grid is
    capped at one resident round and every wave walks its stride more than once, carrying (row, frame) across it.  Bit-identical to
    the product library; the rows either side of every wrap of the stride against the frame oracle."""
    hooks = fm.type_hooks(C.CDLL(fm.hooks_path()))
    for name in ("wekws_hip_fbank_create", "wekws_hip_fbank_destroy", "wekws_hip_fbank_compute_dither"):
        getattr(hooks, name).restype, getattr(hooks, name).argtypes = _capi.SIGNATURES[name]
    B, n, bins, d = 160, 16000, 40, 1.0
    x = synth.synth_pcm(B, n, seed=41, kind="noise")
    pcm = torch.from_numpy(x).cuda()
    cfg = _capi.FbankCfg()
    cfg.num_bins, cfg.sample_rate, cfg.frame_length, cfg.frame_shift, cfg.window = bins, 16000, 400, 160, 0
    h = C.c_void_p()
    assert hooks.wekws_hip_fbank_create(C.byref(cfg), torch.cuda.current_device(), C.byref(h)) == 0
    try:
        feats = torch.empty((B, 98, bins), dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        assert hooks.wekws_hip_fbank_compute_dither(h, pcm.data_ptr(), B, n, feats.data_ptr(), d, dr.SEED, 3, C.c_void_p(stream)) == 0
        torch.cuda.synchronize()
        rec = fm.last(hooks)
    finally:
        hooks.wekws_hip_fbank_destroy(h)
    p = fm.plan(hooks, bins, 16000, 400)
    per_group = p["fw"] * p["waves"]
    assert (rec["B"], rec["nsamp"], rec["nframes"], rec["sample_bytes"], rec["pair_ok"]) == (B, n, 98, 4, 1)
    assert rec["grid"] == rec["resident"] and B * 98 > rec["grid"] * per_group, rec     # one resident round, more than one stride
    got = Fbank(bins, dither=d, seed=dr.SEED)(pcm, first_row=3)
    assert torch.equal(bits(got), bits(feats))
    got = got.cpu().numpy()
    worst = 0.0
    for b in fm.sample_utterances(B, 98, rec["grid"], p["fw"], p["waves"])[:24]:
        frames = dr.dithered_frames(x[b], dr.SEED, 3 + b, 400, 160, d)
        worst = max(worst, float(dr.frame_units(got[b], frames, bins, 16000, 400, 0).max()))
    error_report["dither/full_device_batch"] = worst
    assert worst <= K_FBANK, worst


def test_mfcc_is_the_dct_of_the_dithered_fbank():
    x = dr.case_input(dr.CASES[1])
    pcm = torch.from_numpy(x).cuda()
    mf = Mfcc(80, 80, dither=1.0, seed=dr.SEED)
    fb = Fbank(80, window="povey", dither=1.0, seed=dr.SEED)
    assert torch.equal(bits(mf(pcm, first_row=9)), bits(dct_lifter(fb(pcm, first_row=9), 80, 22.0)))
    assert torch.equal(bits(mf(pcm)), bits(dct_lifter(fb(pcm), 80, 22.0)))                     # both counters at 0 ...
    assert mf.fbank.next_row == fb.next_row == 3                                               # ... and advanced by B
    assert not torch.equal(bits(mf(pcm)), bits(mf(pcm, first_row=0)))                          # rows 3 .. 5 against rows 0 .. 2
    mf.reset_rows()
    assert torch.equal(bits(mf(pcm)), bits(mf(pcm, first_row=0)))


def test_invariances_bit_for_bit():
    lib = _capi.load()
    x = synth.synth_pcm(8, 16000, seed=23, kind="noise")
    x[5] = 0.0
    f32 = torch.from_numpy(x).cuda()
    i16 = f32.to(torch.int16)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # dither = 0 is the plain extractor, through the class and through both dithered entry points
    plain = Fbank(40)
    ref = plain(f32)
    assert torch.equal(bits(Fbank(40, dither=0.0, seed=77)(f32)), bits(ref))
    for fn, t in ((lib.wekws_hip_fbank_compute_dither, f32), (lib.wekws_hip_fbank_compute_dither_i16, i16)):
        out = torch.full_like(ref, 7.0)
        _capi.check(fn(plain._ptr, t.data_ptr(), 8, 16000, out.data_ptr(), 0.0, 77, 3, stream), "compute_dither")
        assert torch.equal(bits(out), bits(ref))
    for bins, window in ((40, "hamming"), (80, "povey")):
        fb = Fbank(bins, window=window, dither=1.0, seed=dr.SEED_HI)
        whole = fb(f32)                                                                        # rows 0 .. 7
        assert fb.next_row == 8 and not torch.equal(bits(whole), bits(Fbank(bins, window=window)(f32)))
        assert torch.equal(bits(fb(f32, first_row=0)), bits(whole))                            # the same call twice
        assert fb.next_row == 8                                                                # (first_row given: the counter stays)
        fb.reset_rows(0)
        parts = torch.cat([fb(f32[:5]), fb(f32[5:])])                                          # 5 + 3 rows, the object's own counter
        assert torch.equal(bits(parts), bits(whole))
        singly = [fb(f32[b:b + 1], first_row=b) for b in reversed(range(8))]                   # one by one, in reverse order
        assert torch.equal(bits(torch.cat(singly[::-1])), bits(whole))
        assert torch.equal(bits(fb(i16, first_row=0)), bits(whole))                            # int16 PCM: the same bits
        fb.reset_rows(0)
        assert torch.equal(bits(fb(f32[:5])), bits(whole[:5]))                                 # reset_rows(0) repeats the first batch
        other = Fbank(bins, window=window, dither=1.0, seed=dr.SEED_HI + 1)(f32)
        assert not torch.equal(bits(other), bits(whole))
    # an odd sample count (the per-sample fetch) draws the same noise: the frames it shares with the even signal are the same bits
    fb = Fbank(40, dither=1.0, seed=dr.SEED)
    assert torch.equal(bits(fb(f32[:, :15999].contiguous(), first_row=0)[:, :97]), bits(fb(f32, first_row=0)[:, :97]))


def test_bit_identical_beside_a_model_forward_on_another_stream():
    """tests/test_hip_fbank.py's tenant case for the dithered kernels: an MDTC forward on another stream puts MFMA waves on the SIMDs
    of the fbank waves (pk_safe.hip.h); every frame must equal the solo run."""
    from tests.test_hip_parity import build
    from wekws_amd import pack
    cfg = dict(synth.MODEL_CONFIGS["mdtc_h64"])
    model = build(cfg, synth.synth_state_dict(pack.model_spec(cfg), 11))
    x = torch.from_numpy(synth.synth_feats(512, 98, cfg["input_dim"], seed=4)).cuda()
    pcm = torch.from_numpy(synth.synth_pcm(768, 16000, seed=5, kind="noise")).cuda()
    fbs = [Fbank(40, dither=1.0, seed=dr.SEED), Fbank(80, window="povey", dither=1.0, seed=dr.SEED)]
    ref = [fb(pcm, first_row=0).clone() for fb in fbs]
    y0 = model(x)[0].clone()
    torch.cuda.synchronize()
    s_fb, s_md = torch.cuda.Stream(), torch.cuda.Stream()
    bad = 0
    for _ in range(12):
        with torch.cuda.stream(s_md):
            for _ in range(6):
                y, _c = model(x)
        with torch.cuda.stream(s_fb):
            got = [[fb(pcm, first_row=0) for _ in range(2)] for fb in fbs]
        torch.cuda.synchronize()
        bad += sum(int((bits(g) != bits(r)).any(dim=-1).sum().item()) for gs, r in zip(got, ref) for g in gs)
        assert torch.equal(bits(y), bits(y0))
    assert bad == 0, f"{bad} frames differ from the solo run"


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_refusals_launch_nothing(bad):
    lib = _capi.load()
    f32 = torch.from_numpy(synth.synth_pcm(2, 16000, seed=1, kind="noise")).cuda()
    fb = Fbank(40, dither=bad, seed=1)
    with pytest.raises(_capi.HipLibraryError, match="dither"):
        fb(f32)
    with pytest.raises(_capi.HipLibraryError, match="dither"):
        Mfcc(80, 80, dither=bad)(f32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fn, t in ((lib.wekws_hip_fbank_compute_dither, f32), (lib.wekws_hip_fbank_compute_dither_i16, f32.to(torch.int16))):
        out = torch.full((2, 98, 40), 7.0, device="cuda")
        assert fn(fb._ptr, t.data_ptr(), 2, 16000, out.data_ptr(), bad, 1, 0, stream) == -1
        assert "dither" in _capi.last_error()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
