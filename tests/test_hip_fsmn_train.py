"""GPU: wekws_amd.model.fsmn -- ``fsmn_memory`` and ``FSMNBlock`` on the device against the torch path and the float64 oracle,
the block swap inside an ``FSMN``, three ``TrainExecutor`` steps with device blocks against torch blocks (float32 and float64),
no host read in the step, and the trained state dict served by the packed inference model."""
import copy

import numpy as np
import pytest
import torch

from tests import fsmn_memory_matrix as fm
from tests.helpers import pow2_at_or_above, tol_for
from tests.train_step import HYPER, _Counter
from wekws_amd.model import fsmn

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = (20, 12, 2, 16, 8, 3, 1, 1, 1, 12, 7)      # input 20, affines 12, 2 units, linear 16, proj 8, lorder 3, rorder 1, 7 classes
TINY_CFG = dict(input_dim=20, output_dim=7, hidden_dim=8, preprocessing=dict(type="none"),
                backbone=dict(type="fsmn", input_affine_dim=12, num_layers=2, linear_dim=16, proj_dim=8, left_order=3, right_order=1,
                              left_stride=1, right_stride=1, output_affine_dim=12),
                classifier=dict(type="identity", dropout=0.1), activation=dict(type="identity"))


class TorchBlock(torch.nn.Module):
    """A memory block that is not the package's: the parameters of ``block`` under torch's own ops, whatever the device.  It has
    the attributes use_device_memory_blocks looks for and nothing else in common with FSMNBlock."""

    def __init__(self, block):
        super().__init__()
        self.lorder, self.rorder, self.lstride, self.rstride = block.lorder, block.rorder, block.lstride, block.rstride
        self.conv_left, self.conv_right = block.conv_left, block.conv_right

    def forward(self, input):
        x, in_cache = input if isinstance(input, tuple) else (input, torch.zeros(0, 0, 0, 0))
        pad = (self.lorder - 1) * self.lstride + self.rorder * self.rstride
        return fsmn.FSMNBlock._forward_torch(self, x, in_cache, pad)


def torch_blocks(model):
    """Every FSMNBlock of ``model`` replaced by a TorchBlock over the same parameters."""
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, fsmn.FSMNBlock):
                setattr(parent, name, TorchBlock(child))
    return model


def _block_results(block, c, dtype=torch.float32):
    D = c["x"].shape[2]
    x = torch.from_numpy(c["x"].copy()).cuda().to(dtype).requires_grad_()
    y, cache = block((x, torch.zeros(0, 0, 0, 0)))
    y.backward(torch.from_numpy(c["g"].copy()).cuda().to(dtype))
    out = dict(y=y.detach(), dx=x.grad, dwl=block.conv_left.weight.grad.reshape(D, -1), dwr=block.conv_right.weight.grad.reshape(D, -1))
    return {k: v.cpu().numpy() for k, v in out.items()}, cache


@pytest.mark.parametrize("name", ["g_mid", "g_stride", "d130", "t33_long", "fold9"])
def test_device_block_and_torch_block_against_the_oracle(name):
    c = fm.load_case(name)
    D, lorder, rorder = c["x"].shape[2], c["wl"].shape[1], c["wr"].shape[1]
    block = fsmn.FSMNBlock(D, D, lorder, rorder, c["lstride"], c["rstride"]).cuda()
    with torch.no_grad():
        block.conv_left.weight.copy_(torch.from_numpy(c["wl"].copy()).view(D, 1, lorder, 1))
        block.conv_right.weight.copy_(torch.from_numpy(c["wr"].copy()).view(D, 1, rorder, 1))
    twin = TorchBlock(copy.deepcopy(block))
    got, cache = _block_results(block, c)
    want, cache_t = _block_results(twin, c)
    assert torch.equal(cache, cache_t) and cache.shape == (c["x"].shape[0], D, fm.fr.window(lorder, rorder, c["lstride"], c["rstride"]) - 1, 1)
    ud, bad_d = fm.units(name, got)
    ut, bad_t = fm.units(name, want)
    print(f"{name}: device {ud}  torch on the device {ut}")
    assert not bad_d and not bad_t
    assert all(ud[k] <= fm.BARS[k] for k in ud), ud
    # the plain function on non-contiguous inputs: the same bits as the block
    xt = torch.from_numpy(c["x"].copy()).cuda().transpose(0, 1).contiguous().transpose(0, 1)
    assert not xt.is_contiguous() or xt.shape[0] == 1 or xt.shape[1] == 1
    y = fsmn.fsmn_memory(xt, block.conv_left.weight, block.conv_right.weight, c["lstride"], c["rstride"])
    assert np.array_equal(y.detach().cpu().numpy().view(np.int32), got["y"].view(np.int32))


def test_only_the_gradients_asked_for():
    c = fm.load_case("g_small")
    x = torch.from_numpy(c["x"].copy()).cuda()
    wl = torch.from_numpy(c["wl"].copy()).cuda().requires_grad_()
    wr = torch.from_numpy(c["wr"].copy()).cuda().requires_grad_()
    g = torch.from_numpy(c["g"].copy()).cuda()
    fsmn.fsmn_memory(x, wl, wr).backward(g)                                    # x wants nothing
    ref, _ = fm.oracle("g_small")
    assert x.grad is None and wl.grad.shape == wl.shape
    assert np.allclose(wl.grad.cpu().numpy(), ref["dwl"], rtol=1e-5, atol=1e-6) and np.allclose(wr.grad.cpu().numpy(), ref["dwr"], rtol=1e-5, atol=1e-6)
    x2 = x.clone().requires_grad_()
    fsmn.fsmn_memory(x2, wl.detach(), wr.detach()).backward(g)                 # the taps want nothing
    assert np.allclose(x2.grad.cpu().numpy(), ref["dx"], rtol=1e-5, atol=1e-6)
    with torch.no_grad():
        y = fsmn.fsmn_memory(x, wl, wr)
    assert not y.requires_grad


def test_swapping_blocks_leaves_the_state_dict_alone():
    torch.manual_seed(11)
    model = torch_blocks(fsmn.FSMN(*TINY)).cuda()
    params = list(model.parameters())
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(3, 9, 20, device="cuda")
    with torch.no_grad():
        y_torch, cache_torch = model(x)
    assert fsmn.use_device_memory_blocks(model) == 2
    assert all(type(u[1]) is fsmn.FSMNBlock for u in model.fsmn)
    after = model.state_dict()
    assert list(after) == list(sd) and all(torch.equal(after[k], sd[k]) for k in sd)
    assert all(a is b for a, b in zip(model.parameters(), params))
    with torch.no_grad():
        y, cache = model(x)
    # a cache is the tail of a block's input: the first unit's is bit for bit the same, the next unit's follows the first
    # block's output, which the two paths round differently
    assert torch.equal(cache[..., 0], cache_torch[..., 0])
    for got, want in ((cache, cache_torch), (y, y_torch)):
        assert float((got - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))


def _loader(sizes, T, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(sizes):
        feats = rng.standard_normal((n, T, 20)).astype(np.float32)
        lengths = rng.integers(T // 2, T + 1, n).astype(np.int32)
        lengths[0] = T
        target = rng.integers(1, 7, (n, 3)).astype(np.int64)
        tl = rng.integers(1, 4, n).astype(np.int32)                            # three labels need at most five frames: feasible
        out.append(dict(keys=[f"utt{i}_{j}" for j in range(n)], feats=torch.from_numpy(feats), target=torch.from_numpy(target),
                        feats_lengths=torch.from_numpy(lengths), target_lengths=torch.from_numpy(tl)))
    return out


class _Float64(torch.nn.Module):
    """A float64 model behind the float32 interface of the device criterion."""

    def __init__(self, model):
        super().__init__()
        self.model = model.double()

    def forward(self, x):
        y, c = self.model(x.double())
        return y.float(), c


ARGS = {"criterion": "ctc", "grad_clip": 5.0, "log_interval": 100}


def _distance(a, b, start, ref):
    """The worst |a - b| over the parameters in units of U (|start| + |ref - start|): the scale of tests/optim_matrix.py's p'."""
    worst = 0.0
    for pa, pb, ps, pr in zip(a, b, start, ref):
        pa, pb, ps, pr = (t.detach().double().cpu().numpy() for t in (pa, pb, ps, pr))
        den = U * (np.abs(ps) + np.abs(pr - ps))
        err = np.abs(pa - pb)
        assert np.isfinite(err).all() and not np.any(err[den == 0])
        worst = max(worst, float((err[den > 0] / den[den > 0]).max()))
    return worst


def test_three_training_steps_with_device_blocks_and_with_torch_blocks(error_report):
    """Three TrainExecutor steps (ctc criterion, ClipAdam) from one initialisation: with device blocks, with torch blocks in
    float32, and with torch blocks in float64 (torch.optim.Adam and clip_grad_norm_ there: ClipAdam is float32).  The bound on
    the distance between the first two is pow2_at_or_above(4 x the float32 torch path's distance from the float64 run), in
    units of 2^-24 (|p0| + |p64 - p0|) per element.  Measured on MI355X: the float32 torch path is 54.00 units from the float64
    run, so the bound is 256; device blocks are 18.57 units from torch blocks."""
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(7)
    base = fsmn.FSMN(*TINY)
    loader = _loader((6, 8, 5), 12, 31)
    start = [p.detach().clone() for p in base.parameters()]

    m_dev = copy.deepcopy(base).cuda()
    assert all(type(u[1]) is fsmn.FSMNBlock for u in m_dev.fsmn)
    m_t32 = torch_blocks(copy.deepcopy(base)).cuda()
    m_t64 = _Float64(torch_blocks(copy.deepcopy(base))).cuda()
    TrainExecutor().train(m_dev, ClipAdam(m_dev.parameters(), **HYPER), loader, "cuda", None, ARGS)
    TrainExecutor().train(m_t32, ClipAdam(m_t32.parameters(), **HYPER), loader, "cuda", None, ARGS)
    TrainExecutor().train(m_t64, torch.optim.Adam(m_t64.parameters(), **HYPER), loader, "cuda", None, ARGS)
    p_dev, p_t32, p_t64 = (list(m.parameters()) for m in (m_dev, m_t32, m_t64))
    assert all(p.dtype == torch.float64 for p in p_t64)
    assert any(not torch.equal(p.cpu(), s) for p, s in zip(p_dev, start))
    d_ref = _distance(p_t32, p_t64, start, p_t64)
    d_dev = _distance(p_dev, p_t32, start, p_t64)
    bound = pow2_at_or_above(4 * d_ref)
    print(f"float32 torch path from float64: {d_ref:.2f} units -> bound {bound}; device blocks from torch blocks: {d_dev:.2f} units")
    error_report["fsmn_train/torch32_from_float64"] = d_ref
    error_report["fsmn_train/device_from_torch32"] = d_dev
    assert d_dev <= bound, (d_dev, d_ref, bound)


def test_training_step_reads_nothing_on_the_host(monkeypatch):
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(8)
    model = fsmn.FSMN(*TINY).cuda()
    start = [p.detach().clone() for p in model.parameters()]
    loader = _loader((6, 8, 5), 12, 32)
    opt = ClipAdam(model.parameters(), **HYPER)
    TrainExecutor().train(model, opt, loader[:1], "cuda", None, ARGS)           # (the first call of a kernel loads its code object)
    torch.cuda.synchronize()
    with monkeypatch.context() as mp:
        counter = _Counter(mp)
        TrainExecutor().train(model, opt, loader, "cuda", None, ARGS)
        reads = list(counter.calls)
    assert reads == [], reads
    assert int(opt.steps) == 1 + len(loader) and int(opt.skipped_steps) == 0
    assert any(not torch.equal(p, s) for p, s in zip(model.parameters(), start))


def test_trained_state_dict_is_served_by_the_packed_model():
    """train -> pack -> serve: the trained FSMN's state dict loads into init_model's packed KWSModel, whose forward_softmax
    agrees with the torch module's softmax at the bar of tests/test_hip_parity.py's goldens."""
    from wekws_amd.model.kws_model import init_model
    from wekws_amd.optim import ClipAdam
    from wekws_amd.utils.executor import TrainExecutor
    torch.manual_seed(9)
    model = fsmn.FSMN(*TINY).cuda()
    TrainExecutor().train(model, ClipAdam(model.parameters(), **HYPER), _loader((6, 8, 5), 12, 33), "cuda", None, ARGS)
    packed = init_model(TINY_CFG)
    packed.load_state_dict({"backbone." + k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    packed = packed.cuda().eval()
    x = torch.randn(4, 30, 20, device="cuda")
    model.eval()
    with torch.no_grad():
        logits, cache = model(x)
        want = torch.softmax(logits, dim=-1).cpu().numpy()
    y, pc = packed.forward_softmax(x)
    err = float(np.abs(y.cpu().numpy() - want).max())
    print(f"packed forward_softmax vs the trained torch module: max|err| = {err:.2e} (bar {tol_for(want):.1e})")
    assert y.shape == want.shape and err <= tol_for(want)
