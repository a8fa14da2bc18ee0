"""GPU: the validation criterion (wekws_amd.criterion -> wekws_hip_criterion_* / wekws_hip_ctc_loss / wekws_hip_ctc_edit_distance)
on the case matrix of tests/criterion_matrix.py: comparisons bit-exact against the live reference's goldens, losses within the
derived bar of the float64 oracle, the same bits on every run and for every split of the batch, nothing written beside an
output buffer, Executor.test on packed models, and the same bits beside an MFMA tenant."""
import os

import numpy as np
import pytest
import torch

from tests import criterion_matrix as cm
from tests import criterion_ref as cr
from tests.test_hip_tenants import tenant  # noqa: F401  (the MFMA tenants of the second stream)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64          # sentinel elements either side of every buffer the binding allocates


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "criterion_golden.npz"))


class _GuardedTorch:
    """Stands in for the `torch` module inside wekws_amd.criterion: every buffer the binding allocates for the library
    (torch.empty / empty_like) is the middle of a larger one filled with a sentinel, checked after the call."""

    def __init__(self):
        self.bufs = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _guarded(self, shape, dtype, device):
        n = int(np.prod(shape)) if len(shape) else 1
        fill = 0x5A if dtype == torch.uint8 else (-77 if dtype in (torch.int32, torch.int64) else -12345.0)
        buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=device)
        self.bufs.append((buf, n, fill))
        return buf[PAD:PAD + n].view(shape)

    def empty(self, shape, dtype=None, device=None):
        return self._guarded(tuple(shape), dtype, device)

    def empty_like(self, x):
        return self._guarded(tuple(x.shape), x.dtype, x.device)

    def check(self):
        assert self.bufs
        for buf, n, fill in self.bufs:
            assert bool((buf[:PAD] == fill).all()) and bool((buf[PAD + n:] == fill).all()), (buf.dtype, n)


@pytest.fixture()
def crit(monkeypatch):
    from wekws_amd import criterion
    g = _GuardedTorch()
    monkeypatch.setattr(criterion, "torch", g)
    yield criterion
    g.check()


def _dev(c):
    return {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def _bits(t):
    t = t.cpu().numpy()
    return t.view(np.int32) if t.dtype == np.float32 else (t.view(np.int64) if t.dtype == np.float64 else t)


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _splits(B):
    return [B] if B < 2 else sorted({1, B // 2, B - 1})


def _record(error_report, kind, u):
    key = f"criterion/{kind}_units"
    error_report[key] = max(u, error_report.get(key, 0.0))


@pytest.mark.parametrize("name", cm.case_names("max_pooling"))
def test_max_pooling(crit, gold, error_report, name):
    c = cm.load_case("max_pooling", name, gold)
    d = _dev(c)
    r = crit.max_pooling_loss_device(d["scores"], d["target"], d["lengths"], c["min_duration"])
    o = cr.max_pooling(**c)
    assert np.array_equal(r.pooled.cpu().numpy(), gold[name + "/pooled"], equal_nan=True)     # every bit, NaN payloads apart
    assert np.array_equal(r.correct.cpu().numpy(), gold[name + "/correct"])
    assert int(r.num_correct) == int(gold[name + "/correct"].sum())
    loss, acc = crit.criterion("max_pooling", d["scores"], d["target"], d["lengths"], min_duration=c["min_duration"])
    assert acc == float(gold[name + "/acc"]) == float(r.acc) and loss.dtype == torch.float32 and loss.dim() == 0
    u = max(cm.units(r.loss_terms.cpu().numpy(), o["terms"]), cm.units(r.loss.cpu().numpy(), o["loss"]))
    print(f"{name}: {u:.2f} units (bar {cm.BARS['max_pooling']})")
    _record(error_report, "max_pooling", u)
    assert u <= cm.BARS["max_pooling"]
    assert np.isnan(float(gold[name + "/loss"])) == np.isnan(float(loss)) == bool(np.isnan(o["loss"]))
    # the same bits again, and row by row for every split of the batch
    assert _same(r, crit.max_pooling_loss_device(d["scores"], d["target"], d["lengths"], c["min_duration"]))
    B = c["scores"].shape[0]
    for k in _splits(B):
        if k == B:
            continue
        parts = [crit.max_pooling_loss_device(d["scores"][s], d["target"][s], d["lengths"][s], c["min_duration"])
                 for s in (slice(0, k), slice(k, B))]
        for f in ("pooled", "loss_terms", "correct"):
            assert np.array_equal(_bits(torch.cat([getattr(p, f) for p in parts])), _bits(getattr(r, f))), (name, k, f)


def test_max_pooling_nan_pooled_values_are_nan_where_the_reference_has_them(crit, gold):
    c = cm.load_case("max_pooling", "mp_5x37x3_nan", gold)
    d = _dev(c)
    r = crit.max_pooling_loss_device(d["scores"], d["target"], d["lengths"], c["min_duration"])
    want = gold["mp_5x37x3_nan/pooled"]
    assert np.isnan(want).sum() == 2 and np.array_equal(np.isnan(r.pooled.cpu().numpy()), np.isnan(want))
    assert not np.isnan(want[2]).any() and not np.isnan(want[1]).any()        # NaN in a masked frame / under min_duration
    assert r.correct.cpu().tolist() == gold["mp_5x37x3_nan/correct"].tolist() and r.correct[1].item() == 0


@pytest.mark.parametrize("name", cm.case_names("ce"))
def test_cross_entropy(crit, gold, error_report, name):
    c = cm.load_case("ce", name, gold)
    d = _dev(c)
    r = crit.cross_entropy_device(d["logits"], d["target"])
    o = cr.cross_entropy(**c)
    assert np.array_equal(r.pred.cpu().numpy(), gold[name + "/pred"])
    assert np.array_equal(r.correct.cpu().numpy(), o["correct"])
    loss, acc = crit.criterion("ce", d["logits"], d["target"], None)
    assert acc == float(gold[name + "/acc"]) == float(r.acc)
    u = max(cm.units(r.loss_rows.cpu().numpy(), o["rows"]), cm.units(loss.cpu().numpy(), o["loss"]))
    print(f"{name}: {u:.2f} units (bar {cm.BARS['ce']})")
    _record(error_report, "ce", u)
    assert u <= cm.BARS["ce"]
    assert _same(r, crit.cross_entropy_device(d["logits"], d["target"]))
    B = c["logits"].shape[0]
    for k in _splits(B):
        if k == B:
            continue
        parts = [crit.cross_entropy_device(d["logits"][s], d["target"][s]) for s in (slice(0, k), slice(k, B))]
        for f in ("loss_rows", "pred", "correct"):
            assert np.array_equal(_bits(torch.cat([getattr(p, f) for p in parts])), _bits(getattr(r, f))), (name, k, f)


def test_cross_entropy_bad_target_is_nan_and_incorrect(crit):
    x = torch.tensor([[0.0, 1.0, 2.0], [3.0, 1.0, 0.0], [1.0, 5.0, 1.0]], device="cuda")
    r = crit.cross_entropy_device(x, torch.tensor([2, 3, -1], device="cuda"))
    rows = r.loss_rows.cpu().numpy()
    assert np.isfinite(rows[0]) and np.isnan(rows[1]) and np.isnan(rows[2]) and np.isnan(float(r.loss))
    assert r.correct.cpu().tolist() == [1, 0, 0] and r.pred.cpu().tolist() == [2, 0, 1]


@pytest.mark.parametrize("name", cm.case_names("ctc"))
def test_ctc_loss(crit, gold, error_report, name):
    c = cm.load_case("ctc", name, gold)
    d = _dev(c)
    r = crit.ctc_loss_device(d["logits"], d["targets"], d["lengths"], d["target_lengths"])
    o = cr.ctc(**c)
    rows = r.loss_rows.cpu().numpy()
    assert np.array_equal(np.isinf(rows), np.isinf(gold[name + "/rows"])) and not np.isnan(rows).any()
    loss, acc = crit.criterion("ctc", d["logits"], d["targets"], d["lengths"], target_lengths=d["target_lengths"])
    assert acc == 0.0 and np.isinf(float(loss)) == np.isinf(float(gold[name + "/loss"]))
    u = max(cm.units(rows, o["rows"]), cm.units(loss.cpu().numpy(), o["loss"]))
    print(f"{name}: {u:.2f} units (bar {cm.BARS['ctc']})")
    _record(error_report, "ctc", u)
    assert u <= cm.BARS["ctc"]
    assert _same(r, crit.ctc_loss_device(d["logits"], d["targets"], d["lengths"], d["target_lengths"]))
    B = c["logits"].shape[0]
    for k in _splits(B):
        if k == B:
            continue
        parts = [crit.ctc_loss_device(d["logits"][s], d["targets"][s], d["lengths"][s], d["target_lengths"][s])
                 for s in (slice(0, k), slice(k, B))]
        assert np.array_equal(_bits(torch.cat([p.loss_rows for p in parts])), _bits(r.loss_rows)), (name, k)


def test_ctc_bad_label_is_nan(crit):
    x = torch.zeros(3, 4, 5, device="cuda")
    tg = torch.tensor([[1, 2], [5, 1], [0, 1]], device="cuda")                   # 5 >= V; 0 is the blank
    r = crit.ctc_loss_device(x, tg, torch.tensor([4, 4, 4], device="cuda"), torch.tensor([2, 2, 2], device="cuda"))
    rows = r.loss_rows.cpu().numpy()
    assert np.isfinite(rows[0]) and np.isnan(rows[1]) and np.isnan(rows[2]) and np.isnan(float(r.loss))


@pytest.mark.parametrize("name", cm.case_names("acc"))
def test_utterance_accuracy(crit, gold, error_report, name):
    c = cm.load_case("acc", name, gold)
    d = _dev(c)
    r = crit.ctc_loss_device(d["logits"], d["targets"], d["lengths"], d["target_lengths"], need_acc=True)
    assert np.array_equal(r.distances.cpu().numpy(), gold[name + "/dist"])
    assert r.totals.cpu().tolist() == gold[name + "/totals"].tolist()
    loss, acc = crit.criterion("ctc", d["logits"], d["targets"], d["lengths"], target_lengths=d["target_lengths"], validation=True)
    assert acc == float(gold[name + "/acc"]) == float(r.acc)
    u = max(cm.units(r.loss_rows.cpu().numpy(), cr.ctc(**c)["rows"]), cm.units(loss.cpu().numpy(), cr.ctc(**c)["loss"]))
    _record(error_report, "ctc", u)
    assert u <= cm.BARS["ctc"]
    assert _same(r, crit.ctc_loss_device(d["logits"], d["targets"], d["lengths"], d["target_lengths"], need_acc=True))
    B = c["logits"].shape[0]
    parts = [crit.ctc_loss_device(d["logits"][s], d["targets"][s], d["lengths"][s], d["target_lengths"][s], need_acc=True)
             for s in (slice(0, 3), slice(3, B))]
    assert np.array_equal(torch.cat([p.distances for p in parts]).cpu().numpy(), gold[name + "/dist"])
    # no label in the whole batch: the reference's ZeroDivisionError; the device form carries NaN
    z = torch.zeros_like(d["target_lengths"])
    with pytest.raises(ZeroDivisionError):
        crit.criterion("ctc", d["logits"], d["targets"], d["lengths"], target_lengths=z, validation=True)
    assert np.isnan(float(crit.ctc_loss_device(d["logits"], d["targets"], d["lengths"], z, need_acc=True).acc))


def test_edit_distance_beyond_one_wave():
    """Labels and hypotheses longer than the wave's 64 lanes, through the C ABI on hand-made beam records."""
    import ctypes
    from wekws_amd import _capi
    from wekws_amd.criterion import _PATH_BEAM, _decoder
    rng = np.random.default_rng(7)
    cap, B, Lmax = 150, 5, 100
    hd = _decoder(torch.device("cuda", 0), 16)
    bb = hd.beam_bytes(cap)
    hyps = [rng.integers(1, 6, n).tolist() for n in (0, 1, 70, 150, 97)]
    labs = [rng.integers(1, 6, n).tolist() for n in (3, 0, 100, 66, 97)]
    labs[4] = list(hyps[4])
    labs[4][50] = 9
    rec = np.full((B, bb), 0x5A, np.uint8)
    tok_off = 8 + 4 * ((_PATH_BEAM + 1) & ~1) + 16 * _PATH_BEAM
    for b, h in enumerate(hyps):
        rec[b, :4].view(np.int32)[0] = 1 if b else 0                 # row 0: an empty record (count 0)
        rec[b, 8:12].view(np.int32)[0] = len(h)
        rec[b, tok_off:tok_off + 4 * len(h)].view(np.int32)[:] = h
    targets = np.zeros((B, Lmax), np.int32)
    for b, l in enumerate(labs):
        targets[b, :len(l)] = l
    tl = np.array([len(l) for l in labs], np.int32)
    out = torch.full((B + 2 * PAD,), -77, dtype=torch.int32, device="cuda")
    tot = torch.full((2 + 2 * PAD,), -77, dtype=torch.int32, device="cuda")
    d_rec, d_tg, d_tl = torch.from_numpy(rec).cuda(), torch.from_numpy(targets).cuda(), torch.from_numpy(tl).cuda()   # kept alive
    _capi.check(_capi.load().wekws_hip_ctc_edit_distance(
        d_rec.data_ptr(), _PATH_BEAM, cap, B, d_tg.data_ptr(), Lmax, d_tl.data_ptr(), out[PAD:].data_ptr(), tot[PAD:].data_ptr(),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "wekws_hip_ctc_edit_distance")
    want = [cr.edit_distance(l, h) for l, h in zip(labs, hyps)]
    assert want[4] == 1 and out[PAD:PAD + B].cpu().tolist() == want
    assert tot[PAD:PAD + 2].cpu().tolist() == [int(tl.sum()), sum(w for w, l in zip(want, labs) if l)]
    for buf, n in ((out, B), (tot, 2)):
        assert bool((buf[:PAD] == -77).all()) and bool((buf[PAD + n:] == -77).all())


def _loader(feats, targets, lengths, target_lengths, sizes):
    out, b0 = [], 0
    for n in sizes:
        s = slice(b0, b0 + n)
        out.append(dict(keys=[f"utt{i}" for i in range(b0, b0 + n)], feats=torch.from_numpy(feats[s]),
                        target=torch.from_numpy(targets[s]), feats_lengths=torch.from_numpy(lengths[s]),
                        target_lengths=torch.from_numpy(target_lengths[s])))
        b0 += n
    return out


def test_executor_on_a_max_pooling_keyword_head():
    """Executor.test on a packed DS-TCN keyword model against the same loop with the oracle criterion on the oracle's
    posteriors.  Bar: -log is 1 / p steep, so a posterior error E moves a batch loss by at most K E / min(pooled); E is the
    1e-4 of the forward's own parity bar (tests/test_hip_parity.py POSTERIOR_TOL)."""
    from oracle import kws_oracle
    from tests.test_hip_parity import build
    from wekws_amd import pack
    from wekws_amd.utils import synth
    from wekws_amd.utils.executor import Executor
    cfg = dict(synth.MODEL_CONFIGS["ds_tcn_h64"])
    sd = synth.synth_state_dict(pack.model_spec(cfg), 1234)
    model = build(cfg, sd)
    K, T, sizes = int(cfg["output_dim"]), 40, (9, 9, 5)
    B = sum(sizes)
    rng = np.random.default_rng(4)
    feats = synth.synth_feats(B, T, cfg["input_dim"], seed=31)
    lengths = rng.integers(1, T + 1, B).astype(np.int32)
    lengths[[0, 9, 18]] = T                                          # the reference needs a full-length row per batch
    targets = rng.integers(-1, K, (B, 1)).astype(np.int64)
    tl = np.ones(B, np.int32)
    loader = _loader(feats, targets, lengths, tl, sizes)
    got = Executor().test(model, loader, "cuda", {"criterion": "max_pooling"})
    batches, slack, b0 = [], 0.0, 0
    for n in sizes:
        s = slice(b0, b0 + n)
        y = kws_oracle.forward(cfg, sd, feats[s], None)[0]
        o = cr.max_pooling(y, targets[s, 0], lengths[s], 0)
        batches.append((np.float32(o["loss"]), o["acc"], n))
        slack = max(slack, K * 1e-4 / float(o["pooled"].min()))
        b0 += n
    want = cr.executor_loop(batches)
    print("executor max_pooling", got, want, slack)
    assert abs(got[0] - want[0]) <= slack + 1e-6 * abs(want[0]) and got[1] == want[1], (got, want, slack)


def test_executor_on_an_fsmn_ctc_head():
    """Executor.test with the ctc criterion (loss and utterance accuracy) on the FSMN CTC model of
    tests/golden/onnx/fsmn_small_ctc.onnx, its logits taken before the exported softmax.  Bar: a logit error E moves every
    log-probability by at most 2 E (the logit and the log-sum-exp), a row's loss by 2 E len; E is measured here against the
    oracle's logits and held to the forward's bar."""
    from oracle import kws_oracle
    from tests.test_hip_parity import build
    from wekws_amd.utils.executor import Executor
    from wekws_amd.utils.onnx_lower import load_model_file
    cfg, sd, _ = load_model_file(os.path.join(ROOT, "tests", "golden", "onnx", "fsmn_small_ctc.onnx"))
    cfg.pop("_exported_softmax", None)
    model = build(cfg, sd)
    V, T, sizes = int(cfg["output_dim"]), 30, (5, 4)
    B = sum(sizes)
    rng = np.random.default_rng(5)
    from wekws_amd.utils import synth
    feats = synth.synth_feats(B, T, cfg["input_dim"], seed=41)
    lengths = rng.integers(12, T + 1, B).astype(np.int32)
    tl = rng.integers(0, 4, B).astype(np.int32)
    tl[0], tl[5] = 3, 2                                             # each batch holds a label: the reference divides by their count
    targets = rng.integers(1, V, (B, 3)).astype(np.int64)
    loader = _loader(feats, targets, lengths, tl, sizes)
    got = Executor().test(model, loader, "cuda", {"criterion": "ctc"})
    batches, slack, b0 = [], 0.0, 0
    for n in sizes:
        s = slice(b0, b0 + n)
        y = kws_oracle.forward(cfg, sd, feats[s], None)[0]
        e = float(np.abs(model(torch.from_numpy(feats[s]).cuda())[0].cpu().numpy() - y).max())
        assert e <= 1e-4 * max(1.0, float(np.abs(y).max())), e
        o = cr.ctc(y, targets[s], lengths[s], tl[s])
        a = cr.utterance_accuracy(y, targets[s], lengths[s], tl[s])
        batches.append((np.float32(o["loss"]), a["acc"], n))
        slack = max(slack, 2 * e * T)
        b0 += n
    want = cr.executor_loop(batches)
    print("executor ctc", got, want, slack)
    assert abs(got[0] - want[0]) <= slack + 1e-6 * abs(want[0]) and got[1] == want[1], (got, want, slack)


def test_criterion_beside_an_mfma_tenant(tenant, gold):  # noqa: F811
    """Every criterion kernel on one stream, an MFMA-heavy forward on another: bit-identical to the solo run."""
    from wekws_amd import criterion as crit
    mp = _dev(cm.load_case("max_pooling", "mp_300x3x2_md2", gold))
    ce = _dev(cm.load_case("ce", "ce_300x2599", gold))
    ct = _dev(cm.load_case("ctc", "ctc_v40_t300", gold))
    ac = _dev(cm.load_case("acc", "acc_v16_t30", gold))
    big = torch.from_numpy(np.random.default_rng(9).random((2048, 98, 2), dtype=np.float32)).cuda()
    big_t = torch.zeros(2048, dtype=torch.int32, device="cuda")

    def work():
        out = list(crit.max_pooling_loss_device(mp["scores"], mp["target"], mp["lengths"], mp["min_duration"]))
        out += list(crit.max_pooling_loss_device(big, big_t, None, 0))
        out += list(crit.cross_entropy_device(ce["logits"], ce["target"]))
        out += list(crit.ctc_loss_device(ct["logits"], ct["targets"], ct["lengths"], ct["target_lengths"]))
        out += list(crit.ctc_loss_device(ac["logits"], ac["targets"], ac["lengths"], ac["target_lengths"], need_acc=True))
        return out

    solo = [None if t is None else t.clone() for t in work()]
    tm, tx = tenant
    torch.cuda.synchronize()
    s_a, s_b = torch.cuda.Stream(), torch.cuda.Stream()
    for rnd in range(6):
        with torch.cuda.stream(s_b):
            for _ in range(8):
                tm(tx)
        with torch.cuda.stream(s_a):
            got = work()
        torch.cuda.synchronize()
        assert _same(got, solo), rnd
