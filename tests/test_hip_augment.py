"""GPU: the augmentation stages (wekws_hip_reverb_*, wekws_hip_noise_*, wekws_hip_spec_mask: wekws_amd.augment) against the
float64 restatements of tests/augment_ref.py, at the bars recorded there: K_REVERB units of 2^-24 |h|_2 |x|_2 per row, K_NOISE
units of 2^-24 (|x| + |g v|) per sample, the masks bit for bit."""
import numpy as np
import pytest
import torch

from tests import augment_ref as AR
from wekws_amd import _capi
from wekws_amd.augment import AddNoise, Reverb, spec_aug

pytestmark = pytest.mark.gpu

DEV = "cuda"
H = AR.HOP
SENTINEL = 12345.0


def bits(t):
    return t.contiguous().view(torch.int32)


def padded(rows, nmax=None, fill=np.nan):
    """(B, nmax) float32 with `fill` behind every row's samples: what lies past a row's length must not be read as signal"""
    nmax = max(r.size for r in rows) if nmax is None else nmax
    out = np.full((len(rows), nmax), fill, dtype=np.float32)
    for b, r in enumerate(rows):
        out[b, :r.size] = r
    return out


def guarded(B, nmax):
    """an output buffer of sentinels with a guard row on either side of the (B, nmax) window the call writes"""
    whole = torch.full((B + 2, nmax), SENTINEL, device=DEV)
    return whole, whole[1:B + 1]


def sentinels_intact(whole, lens):
    got = whole.cpu().numpy()
    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), "a guard row was written"
    for b, n in enumerate(lens):
        assert (got[b + 1, n:] == SENTINEL).all(), f"row {b}: written at or past its {n} samples"


@pytest.fixture(scope="module")
def cases():
    assert _capi.load().wekws_hip_reverb_hop() == H
    xs, hs = AR.reverb_cases()
    return xs, hs, Reverb(hs)


@pytest.fixture(scope="module")
def matrix(cases):
    """every row length with every RIR length in one call: 36 rows"""
    xs, hs, rv = cases
    rows = [(i, j) for i in range(len(xs)) for j in range(len(hs))]
    pcm = torch.from_numpy(padded([xs[i] for i, _ in rows])).to(DEV)
    lens = [xs[i].size for i, _ in rows]
    whole, out = guarded(len(rows), pcm.size(1))
    rv(pcm, [j for _, j in rows], lens, out=out)
    torch.cuda.synchronize()
    return rows, pcm, lens, whole, out


def test_reverb_every_length_pair_within_the_bar(cases, matrix):
    xs, hs, rv = cases
    rows, pcm, lens, whole, out = matrix
    assert rv.num_rirs == len(hs) and rv.spectra_bytes == sum(-(-h.size // H) for h in hs) * (H + 1) * 8
    assert rv.workspace_bytes(len(rows), pcm.size(1)) == len(rows) * 3 * (H + 1) * 8 + len(rows) * 4
    sentinels_intact(whole, lens)
    got = out.cpu().numpy()
    worst = 0.0
    for b, (i, j) in enumerate(rows):
        e = AR.reverb_error(got[b, :lens[b]], xs[i], hs[j])
        print(f"n {xs[i].size} L {hs[j].size}: {e:.3f} U")
        worst = max(worst, e)
    print(f"reverb: worst {worst:.3f} U of a bar of {AR.K_REVERB:.2f}")
    assert worst <= AR.K_REVERB


def test_reverb_rows_do_not_depend_on_the_batch_or_the_call(cases, matrix):
    xs, hs, rv = cases
    rows, pcm, lens, whole, out = matrix
    again = rv(pcm, [j for _, j in rows], lens, out=torch.full_like(out, SENTINEL))
    assert torch.equal(bits(again), bits(out))
    for b, (i, j) in enumerate(rows):
        alone = rv(pcm[b:b + 1, :max(lens[b], 1)].contiguous(), [j], [lens[b]])
        assert torch.equal(bits(alone[0, :lens[b]]), bits(out[b, :lens[b]])), (xs[i].size, hs[j].size)


RAGGED_ROWS = (5, 0, 3, 4, 1)          # indices into REVERB_ROWS: 3H, 1, H + 1, 2H + 1, H - 1
RAGGED_RIRS = (5, 5, -1, 2, 0)         # 2H + 1 taps twice (once longer than its row), a copied row, H - 1 taps, one tap


def ragged(cases, poison=None):
    xs, hs, rv = cases
    rows = [xs[i].copy() for i in RAGGED_ROWS]
    if poison is not None:
        rows[3][H + 7] = poison
    pcm = torch.from_numpy(padded(rows)).to(DEV)
    lens = [r.size for r in rows]
    whole, out = guarded(len(rows), pcm.size(1))
    rv(pcm, RAGGED_RIRS, lens, out=out)
    torch.cuda.synchronize()
    sentinels_intact(whole, lens)
    return rows, pcm, lens, out


def test_reverb_ragged_batch(cases):
    xs, hs, rv = cases
    rows, pcm, lens, out = ragged(cases)
    got = out.cpu().numpy()
    for b, j in enumerate(RAGGED_RIRS):
        if j < 0:
            assert torch.equal(bits(out[b, :lens[b]]), bits(pcm[b, :lens[b]])), "a row without an RIR is copied bit for bit"
        else:
            assert AR.reverb_error(got[b, :lens[b]], rows[b], hs[j]) <= AR.K_REVERB
        alone = rv(pcm[b:b + 1, :lens[b]].contiguous(), [j])                       # (without lengths: the whole row)
        assert torch.equal(bits(alone[0]), bits(out[b, :lens[b]]))
    assert torch.equal(bits(ragged(cases)[3]), bits(out))


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_reverb_poisoned_row_is_nan_and_alone(cases, poison):
    clean = ragged(cases)[3]
    rows, pcm, lens, out = ragged(cases, poison)
    assert torch.isnan(out[3, :lens[3]]).all(), "a NaN / Inf among a row's samples makes the whole row NaN"
    for b in (0, 1, 2, 4):
        assert torch.equal(bits(out[b, :lens[b]]), bits(clean[b, :lens[b]]))


def test_reverb_calls_queue_without_a_synchronise(cases):
    """more calls back to back than the ring of row tables holds, with row counts that make its slots grow"""
    xs, hs, rv = cases
    pcm = torch.from_numpy(padded([xs[3]] * 9, fill=0.0)).to(DEV)
    picks = [[(k + b) % len(hs) - (b == 2) * 9 for b in range(1 + (4 * k) % 9)] for k in range(7)]
    picks = [[max(p, -1) for p in row] for row in picks]
    torch.cuda.synchronize()
    queued = [rv(pcm[:len(p)].contiguous(), p) for p in picks]
    torch.cuda.synchronize()
    for p, q in zip(picks, queued):
        one = rv(pcm[:len(p)].contiguous(), p)
        torch.cuda.synchronize()
        assert torch.equal(bits(one), bits(q))


def test_reverb_refusals_launch_nothing(cases):
    xs, hs, rv = cases
    lib = _capi.load()
    pcm = torch.from_numpy(padded([xs[2], xs[3]], fill=0.0)).to(DEV)
    out = torch.full_like(pcm, SENTINEL)
    n = pcm.size(1)

    def call(src, dst, nsamp, rir, B=2, nmax=n):
        ns, r = np.asarray(nsamp, dtype=np.int32), np.asarray(rir, dtype=np.int32)
        return lib.wekws_hip_reverb_apply(rv._ptr, src, B, nmax, ns.ctypes.data, r.ctypes.data, dst, None)

    assert call(pcm.data_ptr(), pcm.data_ptr(), [n, n], [0, 1]) == -1 and "out must not be pcm" in _capi.last_error()
    assert call(pcm.data_ptr(), out.data_ptr(), [n, n + 1], [0, 1]) == -1 and "row 1" in _capi.last_error()
    assert call(pcm.data_ptr(), out.data_ptr(), [n, -1], [0, 1]) == -1
    assert call(pcm.data_ptr(), out.data_ptr(), [n, n], [len(hs), 1]) == -1 and "row 0" in _capi.last_error()
    assert call(pcm.data_ptr(), out.data_ptr(), [n, n], [0, -2]) == -1
    assert call(None, out.data_ptr(), [n, n], [0, 1]) == -1 and call(pcm.data_ptr(), None, [n, n], [0, 1]) == -1
    assert call(pcm.data_ptr(), out.data_ptr(), [n, n], [0, 1], B=-1) == -1
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    with pytest.raises(ValueError):
        rv(pcm.cpu(), [0, 1])
    with pytest.raises(ValueError):
        rv(pcm, [0])
    with pytest.raises(ValueError):
        rv(pcm.double(), [0, 1])
    with pytest.raises(RuntimeError):
        Reverb(hs, device="cpu")
    assert rv(pcm[:0], []).shape == (0, n)


def test_reverb_with_an_fp16_rir_misses_the_bar(cases):
    """the negative control of K_REVERB: the same cases with the normalised RIR rounded to fp16 (a one-tap RIR normalises to +-1
    and survives the rounding: L >= 64 only)"""
    xs, hs, _ = cases
    long = [j for j, h in enumerate(hs) if h.size >= 64]
    rv16 = Reverb([AR.normalised(hs[j]).astype(np.float16).astype(np.float32) for j in long])
    rows = [(i, k) for i in range(len(xs)) for k in range(len(long))]
    pcm = torch.from_numpy(padded([xs[i] for i, _ in rows])).to(DEV)
    got = rv16(pcm, [k for _, k in rows], [xs[i].size for i, _ in rows]).cpu().numpy()
    errs = [AR.reverb_error(got[b, :xs[i].size], xs[i], hs[long[k]]) for b, (i, k) in enumerate(rows)]
    print(f"fp16 RIR: {min(errs):.1f} .. {max(errs):.1f} U")
    assert min(errs) > AR.K_REVERB


# ---------------------------------------------------------------------------------------------- noise
@pytest.mark.parametrize("scale", [1.0, 32768.0])
def test_noise_within_the_bar(scale):
    bank, rows = AR.noise_bank(), AR.noise_rows(scale)
    nz = AddNoise(bank, pcm_scale=scale)
    assert nz.lengths == [n for _, n, _ in AR.NOISE_BANK]
    rows.append(AR.utterance(2000, 99, scale))                        # and a row without noise
    which = [r for _, r, _, _, _ in AR.NOISE_CASES] + [-1]
    start = [s for _, _, s, _, _ in AR.NOISE_CASES] + [-7]            # (a copied row's draws are not read)
    snr = [d for _, _, _, d, _ in AR.NOISE_CASES] + [float("nan")]
    lens = [r.size for r in rows]
    pcm = torch.from_numpy(padded(rows)).to(DEV)
    out = nz(pcm, which, start, snr, lens)
    got = out.cpu().numpy()
    worst = 0.0
    for b, (n, r, st, d, _) in enumerate(AR.NOISE_CASES):
        e = AR.noise_error(got[b, :n], rows[b], bank[r], st, d, scale)
        print(f"n {n} noise {AR.NOISE_BANK[r][0]} start {st} snr {d}: {e:.2f} units")
        worst = max(worst, e)
    print(f"noise, pcm_scale {scale}: worst {worst:.2f} units of a bar of {AR.K_NOISE:.1f}")
    assert worst <= AR.K_NOISE
    assert torch.equal(bits(out[6, :lens[6]]), bits(pcm[6, :lens[6]])), "a silent noise adds nothing"
    assert torch.equal(bits(out[-1]), bits(pcm[-1])), "a row without noise is copied bit for bit"
    for b, n in enumerate(lens):
        assert torch.equal(bits(out[b, n:]), bits(pcm[b, n:])), "past a row's samples nothing changes"
    # in place, and a second call
    twin = pcm.clone()
    assert nz(twin, which, start, snr, lens, inplace=True) is twin
    assert torch.equal(bits(twin), bits(out)) and torch.equal(bits(nz(pcm, which, start, snr, lens)), bits(out))
    # non-finite samples propagate as the arithmetic has them: the row, not its neighbours
    bad = pcm.clone()
    bad[0, 5] = float("inf")
    got_bad = nz(bad, which, start, snr, lens)
    assert torch.equal(bits(got_bad[1:]), bits(out[1:])) and not torch.isfinite(got_bad[0, 5])


def test_noise_refusals_launch_nothing():
    nz = AddNoise(AR.noise_bank())
    pcm = torch.zeros(2, 3000, device=DEV)
    for which, start, snr, lens in (([2, 0], [2001, 0], [0.0, 0.0], None), ([0, 0], [0, -1], [0.0, 0.0], None),
                                    ([4, 0], [0, 0], [0.0, 0.0], None), ([0, 0], [0, 0], [0.0, float("inf")], None),
                                    ([0, 0], [0, 0], [0.0, 0.0], [3001, 5])):
        out = torch.full_like(pcm, SENTINEL)
        with pytest.raises(_capi.HipLibraryError):
            nz(out, which, start, snr, lens, inplace=True)
        torch.cuda.synchronize()
        assert (out == SENTINEL).all()
    with pytest.raises(_capi.HipLibraryError, match="pcm_scale"):
        AddNoise(AR.noise_bank(), pcm_scale=0.0)(pcm, [0, 0], [0, 0], [0.0, 0.0])
    with pytest.raises(ValueError):
        nz(pcm.cpu(), [0, 0], [0, 0], [0.0, 0.0])


# ---------------------------------------------------------------------------------------------- masks
def mask_feats(B=4, T=23, F=9):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    x[0, 0, 0], x[1, 2, 3], x[2, 22, 8] = -0.0, np.nan, np.inf            # copied as they are
    return x


MASKS = {
    "overlapping": ([[[2, 9], [5, 12]], [[0, 1], [0, 1]], [[22, 23], [21, 23]], [[3, 3], [10, 23]]],
                    [[[1, 4], [3, 6]], [[0, 9], [2, 3]], [[8, 9], [8, 9]], [[4, 4], [0, 1]]], None),
    "no time masks": ([[], [], [], []], [[[1, 4]], [[0, 9]], [[8, 9]], [[4, 4]]], None),
    "no frequency masks": ([[[2, 9]], [[0, 23]], [[22, 23]], [[3, 3]]], [[], [], [], []], None),
    "ragged": ([[[2, 9], [22, 23]], [[9, 10], [0, 1]], [[0, 0], [0, 1]], [[0, 0], [0, 0]]],
               [[[1, 4], [3, 6]], [[0, 9], [2, 3]], [[8, 9], [8, 9]], [[4, 4], [0, 1]]], [23, 10, 1, 0]),
}


@pytest.mark.parametrize("name", sorted(MASKS))
def test_masks_bit_exact(name):
    tm, fm, lengths = MASKS[name]
    x = mask_feats()
    want = AR.spec_aug(x, tm, fm, lengths)
    feats = torch.from_numpy(x).to(DEV)
    got = spec_aug(feats, tm, fm, lengths)
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    assert torch.equal(bits(feats), bits(torch.from_numpy(x).to(DEV))), "the input is left alone"
    assert spec_aug(feats, tm, fm, lengths, inplace=True) is feats
    assert np.array_equal(feats.cpu().numpy().view(np.int32), want.view(np.int32))


def test_masks_refuse_unclipped_masks_and_cpu_tensors():
    feats = torch.from_numpy(mask_feats()).to(DEV)
    keep = feats.clone()
    with pytest.raises(_capi.HipLibraryError, match="row 2"):
        spec_aug(feats, [[[0, 1]], [[0, 1]], [[20, 24]], [[0, 1]]], [[], [], [], []], inplace=True)
    with pytest.raises(_capi.HipLibraryError, match="row 0"):
        spec_aug(feats, [[], [], [], []], [[[8, 10]], [[0, 1]], [[0, 1]], [[0, 1]]], inplace=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(feats), bits(keep))
    with pytest.raises(ValueError):
        spec_aug(feats.cpu(), [[], [], [], []], [[], [], [], []])


# ---------------------------------------------------------------------------------------------- beside a tenant, and the chain
def test_reverb_bit_identical_beside_a_model_forward_on_another_stream():
    """The tenant case of pk_safe.hip.h: the reverb kernels issue no MFMA, a model forward on another stream puts
    MFMA waves on their SIMDs.  Every sample must equal the solo call's."""
    from tests.test_hip_parity import build
    from wekws_amd import pack
    from wekws_amd.utils import synth
    cfg = dict(synth.MODEL_CONFIGS["mdtc_h64"])
    model = build(cfg, synth.synth_state_dict(pack.model_spec(cfg), 11))
    x = torch.from_numpy(synth.synth_feats(512, 98, cfg["input_dim"], seed=4)).cuda()
    pcm = torch.from_numpy(synth.synth_pcm(256, 16000, seed=5, kind="noise")).cuda()
    rv = Reverb([AR.rir(8000, k) for k in range(4)])
    pick = [b % 4 for b in range(256)]
    ref = rv(pcm, pick).clone()
    y0 = model(x)[0].clone()
    torch.cuda.synchronize()
    s_rv, s_md = torch.cuda.Stream(), torch.cuda.Stream()
    out = torch.empty_like(pcm)
    bad = 0
    for _ in range(20):
        with torch.cuda.stream(s_md):
            for _ in range(6):
                y, _c = model(x)
        with torch.cuda.stream(s_rv):
            got = [rv(pcm, pick, out=out).clone() for _ in range(3)]
        torch.cuda.synchronize()
        bad += sum(int((bits(g) != bits(ref)).sum().item()) for g in got)
        assert torch.equal(bits(y), bits(y0))
    assert bad == 0, f"{bad} samples differ from the solo run"


def test_chain_reverb_noise_fbank_against_the_chained_oracles():
    """Reverb -> AddNoise (samples in [-1, 1]) -> x 32768 -> Fbank of 4 short utterances against the float64 restatements chained,
    then the fbank oracle: at the fbank suite's bar (tests/test_hip_fbank.py TOL)"""
    from oracle import fbank_oracle
    from tests.test_hip_fbank import TOL
    from wekws_amd.frontend import Fbank
    lens = [16000, 12001, 9000, 8191]
    xs = [AR.utterance(n, 70 + b) for b, n in enumerate(lens)]
    hs = [AR.rir(4000, 7), AR.rir(9000, 8)]
    bank = AR.noise_bank() + [AR.noise(20000, 9)]
    pick, which, start, snr = [0, 1, 1, 0], [4, 0, 2, 1], [3999, 5, 0, 77], [10.0, 5.0, 0.0, 15.0]
    pcm = torch.from_numpy(padded(xs)).to(DEV)
    wet = Reverb(hs)(pcm, pick, lens)
    noisy = AddNoise(bank, pcm_scale=1.0)(wet, which, start, snr, lens)
    fb = Fbank(40)
    worst = 0.0
    for b, n in enumerate(lens):
        got = fb((noisy[b:b + 1, :n] * 32768.0).contiguous())[0].cpu().numpy()
        want64, _ = AR.add_noise(AR.reverb(xs[b], hs[pick[b]]), bank[which[b]], start[b], snr[b])
        ref = fbank_oracle.fbank(want64 * 32768.0, 40)
        err = float(np.abs(got - ref).max())
        print(f"chain row {b} ({n} samples): max|err| {err:.2e}")
        worst = max(worst, err)
    assert worst <= TOL, worst
