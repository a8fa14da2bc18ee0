"""GPU: the criterion's backward pass (wekws_amd.criterion -> wekws_hip_criterion_*_grad / wekws_hip_ctc_loss_grad) on the case
matrix of tests/criterion_grad_matrix.py: classes exact and values within the derived bar of the float64 oracle, the same bits
on every run, for every split of the batch and beside an MFMA tenant, nothing written beside a buffer, autograd's grad_output
applied exactly, and TrainExecutor against a manual loop."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

from tests import criterion_grad_matrix as gm
from tests.test_criterion_grad_oracle import golden_classes, oracle as _oracle
from tests.test_hip_criterion import _GuardedTorch
from tests.test_hip_tenants import tenant  # noqa: F401  (the MFMA tenants of the second stream)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(k, n) for k in ("max_pooling", "ce", "ctc") for n in gm.case_names(k)]
INPUT = {"max_pooling": "scores", "ce": "logits", "ctc": "logits"}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "criterion_grad_golden.npz"))


@pytest.fixture()
def crit(monkeypatch):
    from wekws_amd import criterion
    g = _GuardedTorch()
    monkeypatch.setattr(criterion, "torch", g)
    yield criterion
    g.check()


@functools.lru_cache(maxsize=None)
def reference(kind, name):
    """The case and the oracle's gradient at divisor 1 (and the rows' nll for ctc), computed once."""
    c = gm.load_case(kind, name)
    g, rows = _oracle(kind, c, 1)
    return c, g, rows


def _dev(c):
    return {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def _rows(d, s):
    return {k: (v[s] if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def _grad(crit, kind, d, **kw):
    if kind == "max_pooling":
        return crit.max_pooling_grad_device(d["scores"], d["target"], d["lengths"], d["min_duration"], **kw)
    if kind == "ce":
        return crit.cross_entropy_grad_device(d["logits"], d["target"], **kw)
    return crit.ctc_loss_grad_device(d["logits"], d["targets"], d["lengths"], d["target_lengths"], **kw)[0]


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _splits(B):
    return [] if B < 2 else sorted({1, B // 2, B - 1})


def _record(error_report, kind, u):
    key = f"criterion_grad/{kind}_units"
    error_report[key] = max(u, error_report.get(key, 0.0))


@pytest.mark.parametrize("kind,name", CASES)
def test_gradient(crit, gold, error_report, kind, name):
    c, o1, rows = reference(kind, name)
    B = gm.batch_size(kind, c)
    d = _dev(c)
    g = _grad(crit, kind, d)                                          # divisor B, upstream NULL: the batch loss's gradient
    gn = g.cpu().numpy()
    assert g.dtype == torch.float32 and gn.shape == o1.shape
    assert np.array_equal(gm.classes(gn), golden_classes(gold, name, gn.shape))       # the reference's own classes
    u = gm.units(kind, gn, o1 / B, B, rows)
    g1 = _grad(crit, kind, d, divisor=1)
    u1 = gm.units(kind, g1.cpu().numpy(), o1, 1, rows)
    print(f"{name}: {u:.2f} units at divisor {B}, {u1:.2f} at divisor 1 (bar {gm.BARS[kind]})")
    _record(error_report, kind, max(u, u1))
    assert max(u, u1) <= gm.BARS[kind]
    assert np.array_equal(_bits(g), _bits(_grad(crit, kind, d)))      # the same bits again
    for k in _splits(B):                                              # a row's gradient depends on that row alone
        parts = [_grad(crit, kind, _rows(d, s), divisor=1) for s in (slice(0, k), slice(k, B))]
        assert np.array_equal(_bits(torch.cat(parts)), _bits(g1)), (name, k)
    g2 = _grad(crit, kind, d, upstream=torch.tensor(2.0, device="cuda"))
    assert np.array_equal(g2.cpu().numpy(), 2.0 * gn, equal_nan=True)                  # exactly twice
    g0 = _grad(crit, kind, d, upstream=0.0).cpu().numpy()
    assert np.array_equal(np.isnan(g0), np.isnan(gn)) and not g0[~np.isnan(gn)].any()
    if kind == "ctc":                                                 # the loss of the gradient call: the forward's bits
        _, lr, ls = crit.ctc_loss_grad_device(d["logits"], d["targets"], d["lengths"], d["target_lengths"])
        r = crit.ctc_loss_device(d["logits"], d["targets"], d["lengths"], d["target_lengths"])
        assert np.array_equal(_bits(lr), _bits(r.loss_rows)) and np.array_equal(_bits(ls), _bits(r.loss))


def test_max_pooling_without_lengths(crit):
    c, _, _ = reference("max_pooling", "mp_4x9x70")
    d = _dev(c)
    full = torch.full_like(d["lengths"], c["scores"].shape[1])
    a = crit.max_pooling_grad_device(d["scores"], d["target"], None, c["min_duration"])
    b = crit.max_pooling_grad_device(d["scores"], d["target"], full, c["min_duration"])
    assert np.array_equal(_bits(a), _bits(b)) and bool(a.any())


def test_bad_labels_and_nan_logits_make_the_row_nan(crit):
    x = torch.tensor([[0.0, 1.0, 2.0], [3.0, 1.0, 0.0], [1.0, 5.0, 1.0], [0.5, float("nan"), 1.0]], device="cuda")
    g = crit.cross_entropy_grad_device(x, torch.tensor([2, 3, -1, 0], device="cuda"), divisor=1).cpu().numpy()
    assert np.isfinite(g[0]).all() and np.isnan(g[1:]).all()
    want = np.exp(x[0].cpu().numpy().astype(np.float64))
    want = want / want.sum() - np.array([0, 0, 1.0])
    assert np.abs(g[0] - want).max() <= gm.BARS["ce"] * 2.0 ** -24
    x = torch.zeros(3, 4, 5, device="cuda")
    tg = torch.tensor([[1, 2], [5, 1], [0, 1]], device="cuda")                   # 5 >= V; 0 is the blank
    ln = torch.tensor([4, 3, 0], device="cuda")
    g, rows, loss = crit.ctc_loss_grad_device(x, tg, ln, torch.tensor([2, 2, 2], device="cuda"), divisor=1)
    g = g.cpu().numpy()
    assert np.isfinite(g[0]).all() and np.isnan(g[1, :3]).all() and not g[1, 3:].any() and not g[2].any()
    assert np.abs(g[0].sum(axis=1)).max() <= 1e-6 and np.isnan(float(loss))


def _case_args(kind, name):
    c, _, _ = reference(kind, name)
    d = _dev(c)
    if kind == "max_pooling":
        return d, (d["target"], d["lengths"]), dict(min_duration=c["min_duration"])
    if kind == "ce":
        return d, (d["target"], None), {}
    return d, (d["targets"], d["lengths"]), dict(target_lengths=d["target_lengths"])


@pytest.mark.parametrize("kind,name", [("max_pooling", "mp_5x37x3_md5"), ("max_pooling", "mpg_ties_6x4x2"), ("ce", "ce_7x12"),
                                       ("ctc", "ctcg_v12_t9"), ("ctc", "ctc_v7_t50")])
def test_autograd(crit, kind, name):
    d, args, kw = _case_args(kind, name)
    x0 = d[INPUT[kind]]
    B = int(x0.shape[0])
    want = _grad(crit, kind, d, divisor=B)
    plain, _ = crit.criterion(kind, x0, *args, **kw)
    assert not plain.requires_grad and plain.grad_fn is None
    x = x0.clone().requires_grad_()
    loss, _ = crit.criterion(kind, x, *args, **kw)
    assert loss.requires_grad and loss.grad_fn is not None and loss.dim() == 0
    assert np.array_equal(_bits(loss), _bits(plain))                  # the loss with a gradient attached: the same bits
    loss.backward()
    assert np.array_equal(_bits(x.grad), _bits(want))
    x2 = x0.clone().requires_grad_()
    r = crit.criterion_device(kind, x2, *args, **kw)
    assert not r.acc.requires_grad and all(not t.requires_grad for t in r[1:] if isinstance(t, torch.Tensor))
    (2 * r.loss).backward()
    assert np.array_equal(x2.grad.cpu().numpy(), 2.0 * want.cpu().numpy(), equal_nan=True)
    with torch.no_grad():
        quiet, _ = crit.criterion(kind, x, *args, **kw)
    assert not quiet.requires_grad and np.array_equal(_bits(quiet), _bits(plain))


class _KeywordHead(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(40, 2)

    def forward(self, x):
        return torch.sigmoid(self.lin(x)), None


class _CtcHead(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(40, 16)

    def forward(self, x):
        return self.lin(x), None


def _loader(kind, sizes, T, seed, infeasible=()):
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(sizes):
        feats = rng.standard_normal((n, T, 40)).astype(np.float32)
        lengths = rng.integers(T // 2, T + 1, n).astype(np.int32)
        lengths[0] = T
        if kind == "max_pooling":
            target = rng.integers(-1, 2, (n, 1)).astype(np.int64)
            tl = np.ones(n, np.int32)
        else:
            target = rng.integers(1, 16, (n, 3)).astype(np.int64)
            tl = rng.integers(0, 4, n).astype(np.int32)
            if i in infeasible:
                lengths[1], tl[1] = 2, 3                                 # three labels in two frames
        out.append(dict(keys=[f"utt{i}_{j}" for j in range(n)], feats=torch.from_numpy(feats), target=torch.from_numpy(target),
                        feats_lengths=torch.from_numpy(lengths), target_lengths=torch.from_numpy(tl)))
    return out


def _manual_epoch(crit, model, opt, loader, kind, clip, min_duration):
    """The same epoch with the raw gradient tensor pushed through logits.backward(g); -> the batches whose step was skipped."""
    skipped = []
    model.train()
    for i, b in enumerate(loader):
        target = b["target"][:, 0] if b["target"].shape[1] == 1 else b["target"]
        feats, target = b["feats"].cuda(), target.cuda()
        ln, tl = b["feats_lengths"].cuda(), b["target_lengths"].cuda()
        logits, _ = model(feats)
        if kind == "max_pooling":
            g = crit.max_pooling_grad_device(logits, target, ln, min_duration)
        else:
            g = crit.ctc_loss_grad_device(logits, target, ln, tl)[0]
        opt.zero_grad()
        logits.backward(g)
        norm = torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
        if torch.isfinite(norm):
            opt.step()
        else:
            skipped.append(i)
    return skipped


def _params(model):
    return [p.detach().cpu().numpy().view(np.int32).copy() for p in model.parameters()]


@pytest.mark.parametrize("kind", ["max_pooling", "ctc"])
def test_train_executor_equals_the_manual_loop(crit, kind):
    from wekws_amd.utils.executor import Executor, TrainExecutor
    torch.manual_seed(3)
    model = (_KeywordHead() if kind == "max_pooling" else _CtcHead()).cuda()
    twin = copy.deepcopy(model)
    start = _params(model)
    loader = _loader(kind, (7, 9, 5), 12, 17, infeasible=(1,))
    args = {"criterion": kind, "min_duration": 2, "grad_clip": 0.05, "log_interval": 100}
    opt = torch.optim.SGD(model.parameters(), lr=0.5)
    TrainExecutor().train(model, opt, loader, "cuda", None, args)
    opt2 = torch.optim.SGD(twin.parameters(), lr=0.5)
    skipped = _manual_epoch(crit, twin, opt2, loader, kind, 0.05, 2)
    assert skipped == ([1] if kind == "ctc" else [])
    got, want = _params(model), _params(twin)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert any(not np.array_equal(a, b) for a, b in zip(got, start))             # it did train
    if kind == "ctc":                                                            # a non-finite norm: the step is skipped
        before = _params(model)
        TrainExecutor().train(model, opt, loader[1:2], "cuda", None, args)
        assert all(np.array_equal(a, b) for a, b in zip(_params(model), before))
        assert any(p.grad is not None and bool(torch.isnan(p.grad).any()) for p in model.parameters())
    with pytest.raises(NotImplementedError):
        Executor().train(model, opt, loader, "cuda", None, args)


def test_gradients_beside_an_mfma_tenant(tenant):  # noqa: F811
    """Every gradient kernel on one stream, an MFMA-heavy forward on another: bit-identical to the solo run."""
    from wekws_amd import criterion as crit
    cases = [("max_pooling", "mp_300x3x2_md2"), ("max_pooling", "mp_4x9x70"), ("ce", "ce_300x2599"), ("ctc", "ctc_v40_t300"),
             ("ctc", "ctc_v2599_t50"), ("ctc", "acc_v16_t30")]
    devs = [(k, _dev(reference(k, n)[0])) for k, n in cases]

    def work():
        return [_grad(crit, k, d) for k, d in devs]

    solo = [t.clone() for t in work()]
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
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, solo)), rnd
