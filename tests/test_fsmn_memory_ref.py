"""CPU: the float64 oracle of the FSMN memory block against the live reference's goldens, the bars of
tests/fsmn_memory_matrix.py recomputed, the torch path of wekws_amd.model.fsmn against the goldens bit for bit, the module
mirror's state-dict layout, the block swap, and the C entry points' plan and refusals (no device needed)."""
import os

import numpy as np
import pytest
import torch

from tests import fsmn_memory_matrix as fm
from tests import fsmn_memory_ref as fr
from tests.helpers import pow2_at_or_above
from wekws_amd import _capi
from wekws_amd.model import fsmn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = (20, 12, 2, 16, 8, 3, 1, 1, 1, 12, 7)
CTC = (400, 140, 4, 250, 128, 10, 2, 1, 1, 140, 2599)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "fsmn_memory_golden.npz"))


def _block(c, dtype=torch.float32):
    D, lorder, rorder = c["x"].shape[2], c["wl"].shape[1], c["wr"].shape[1]
    b = fsmn.FSMNBlock(D, D, lorder, rorder, c["lstride"], c["rstride"]).to(dtype)
    with torch.no_grad():
        b.conv_left.weight.copy_(torch.from_numpy(c["wl"].copy()).to(dtype).view(D, 1, lorder, 1))
        b.conv_right.weight.copy_(torch.from_numpy(c["wr"].copy()).to(dtype).view(D, 1, rorder, 1))
    return b


def torch_path(name, dtype=torch.float32):
    """FSMNBlock's torch path on the CPU: dict(y, cache[, dx, dwl, dwr]) as numpy."""
    c = fm.load_case(name)
    b = _block(c, dtype)
    x = torch.from_numpy(c["x"].copy()).to(dtype).requires_grad_()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                      # the sums' order, and so the recorded units, must not depend on the core count
    try:
        y, cache = b((x, torch.zeros(0, 0, 0, 0, dtype=dtype)))
        out = {"y": y.detach().numpy(), "cache": cache.detach().numpy()}
        if c["backward"]:
            y.backward(torch.from_numpy(c["g"].copy()).to(dtype))
            D = c["x"].shape[2]
            out.update(dx=x.grad.numpy(), dwl=b.conv_left.weight.grad.numpy().reshape(D, -1),
                       dwr=b.conv_right.weight.grad.numpy().reshape(D, -1))
    finally:
        torch.set_num_threads(threads)
    return out


def test_matrix_covers_what_it_says():
    names = fm.case_names()
    assert len(names) == len(set(names)) and set(fm.GOLDEN) <= set(names)
    shapes = [fm.CASES[n] for n in names]
    assert {s[2] for s in shapes} >= {1, 3, 4, 5, 64, 128, 130, 250}
    assert {s[0] for s in shapes} >= {1, 2, 3, 4, 5}
    assert {s[3] for s in shapes} >= set(fm.TAP_SETS.values())
    for taps in fm.TAP_SETS.values():
        w = fr.window(*taps)
        assert {s[1] for s in shapes if s[3] == taps} >= {t for t in (1, 2, w - 1, w, w + 1) if t >= 1}
    assert {s[1] for s in shapes if s[3] == fm.RECIPE_TAPS} >= {63, 64, 65, 131, 127, 128, 129, 259}
    tiles = {fr.grad_tiles(s[0], s[1]) for s in shapes}
    assert any(t <= fr.FOLD_SEGS for t in tiles) and any(t > fr.FOLD_SEGS and t % fr.fold_seg_len(t) for t in tiles)
    assert fm.CASES["recipe"][:3] == (256, 100, 128)
    for n in names:
        B, T, D, taps, _ = fm.CASES[n]
        assert fr.check(B, T, D, *taps)


@pytest.mark.parametrize("name", sorted(fm.GOLDEN))
def test_oracle_equals_the_reference_in_float64(golden, name):
    c = fm.load_case(name)
    for k in ("x", "g", "wl", "wr"):
        assert np.array_equal(golden[f"{name}/{k}"], c[k], equal_nan=True)       # the golden was made from these inputs
    ref, mag = fm.oracle(name)
    for k in ref:
        want = golden[f"{name}/{k}64"]
        assert fm.same_classes(ref[k], want), (name, k)
        fin = np.isfinite(want)
        dev = np.abs(ref[k][fin] - want[fin])
        assert np.all(dev <= 1e-12 * mag[k][fin]), (name, k, float(dev.max()))


@pytest.mark.parametrize("name", sorted(fm.GOLDEN))
def test_torch_path_equals_the_reference_bit_for_bit(golden, name):
    got = torch_path(name)
    y32 = golden[f"{name}/y32"]
    assert np.array_equal(got["y"].view(np.int32), y32.view(np.int32)), name
    assert np.array_equal(got["cache"].view(np.int32), golden[f"{name}/cache32"].view(np.int32)), name
    # (the gradients are autograd's: their last bits follow the order in which it adds the three paths into x, which is not the
    # module's to fix -- they are held to the bars, like the live reference's below)
    ug, bad = fm.units(name, {k: got[k] for k in fm.oracle(name)[0]})
    assert not bad and all(ug[k] <= fm.BARS[k] for k in ug), (name, ug, bad)
    u, bad = fm.units(name, {k: golden[f"{name}/{k}32"] for k in fm.oracle(name)[0]})
    assert not bad and all(u[k] <= fm.BARS[k] for k in u), (name, u, bad)         # the live reference is within its own bars


def test_bars_are_recomputed():
    worst = {k: (0.0, "") for k in fm.QUANTITIES}
    for name in fm.case_names():
        got = torch_path(name)
        u, bad = fm.units(name, {k: got[k] for k in fm.oracle(name)[0]})
        assert not bad, (name, bad)
        for k, v in u.items():
            if v > worst[k][0]:
                worst[k] = (v, name)
    for k in fm.QUANTITIES:
        print(f"{k}: reference's worst units {worst[k][0]:.2f} ({worst[k][1]}) -> bar {pow2_at_or_above(4 * worst[k][0])}")
        assert abs(worst[k][0] - fm.REF_UNITS[k]) < 0.01, (k, worst[k], fm.REF_UNITS[k])
        assert fm.BARS[k] == pow2_at_or_above(4 * worst[k][0]), (k, worst[k], fm.BARS[k])


def test_cache_path_streams_like_one_call():
    """The torch path with a non-empty cache: two chunks with the carried cache give the one-shot output delayed by nothing --
    the reference's streaming contract, which the device path leaves to it."""
    c = fm.load_case("g_stride")
    b = _block(c)
    x = torch.from_numpy(c["x"].copy())
    with torch.no_grad():
        y, _ = b((x, torch.zeros(0, 0, 0, 0)))
        y1, cache = b((x[:, :17], torch.zeros(0, 0, 0, 0)))
        y2, _ = b((x[:, 17:], cache))
    assert torch.equal(torch.cat([y1, y2], 1), y)


@pytest.mark.parametrize("tag,cfg", [("fsmn_tiny", TINY), ("fsmn_ctc", CTC)])
def test_fsmn_state_dict_layout_is_the_references(golden, tag, cfg):
    sd = fsmn.FSMN(*cfg).state_dict()
    assert list(sd) == [str(k) for k in golden[f"{tag}/keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in golden[f"{tag}/shapes"]]
    assert "in_linear1.linear.weight" in sd and "fsmn.0.1.conv_left.weight" in sd


def test_fsmn_forward_shapes_and_cache():
    m = fsmn.FSMN(*TINY)
    x = torch.randn(3, 9, 20)
    y, cache = m(x)
    assert y.shape == (3, 9, 7) and cache.shape == (3, 8, m.padding, 2)
    y1, c1 = m(x[:, :4])
    y2, _ = m(x[:, 4:], c1)
    assert torch.allclose(torch.cat([y1, y2], 1), y, atol=1e-6)


class _ForeignBlock(torch.nn.Module):
    """A memory block that is not ours: recognised by its attributes alone."""

    def __init__(self, dim, lorder, rorder, lstride=1, rstride=1):
        super().__init__()
        self.lorder, self.rorder, self.lstride, self.rstride = lorder, rorder, lstride, rstride
        self.conv_left = torch.nn.Conv2d(dim, dim, [lorder, 1], dilation=[lstride, 1], groups=dim, bias=False)
        self.conv_right = torch.nn.Conv2d(dim, dim, [rorder, 1], dilation=[rstride, 1], groups=dim, bias=False) if rorder > 0 else None


def test_use_device_memory_blocks_shares_parameters_and_skips_what_it_cannot_run():
    net = torch.nn.Sequential(torch.nn.Sequential(torch.nn.Linear(4, 6), _ForeignBlock(6, 3, 1)), _ForeignBlock(6, 2, 0),
                              _ForeignBlock(6, 30, 3), _ForeignBlock(6, 4, 2, 100, 1), fsmn.FSMNBlock(6, 6, 3, 1))
    params = list(net.parameters())
    keys = list(net.state_dict())
    no_right, too_many, too_long, ours = net[1], net[2], net[3], net[4]
    assert fsmn.use_device_memory_blocks(net) == 1
    assert isinstance(net[0][1], fsmn.FSMNBlock) and (net[0][1].lorder, net[0][1].rorder) == (3, 1)
    assert net[1] is no_right and net[2] is too_many and net[3] is too_long and net[4] is ours
    after = list(net.parameters())
    assert len(after) == len(params) and all(a is b for a, b in zip(after, params))      # the very objects an optimiser holds
    assert list(net.state_dict()) == keys
    assert fsmn.use_device_memory_blocks(net) == 0
    y, cache = net[0][1]((torch.randn(2, 5, 6), torch.zeros(0, 0, 0, 0)))                # on the CPU: torch's own ops
    assert y.shape == (2, 5, 6) and cache.shape == (2, 6, 3, 1)


def test_fsmn_memory_refuses_cpu_tensors():
    with pytest.raises(ValueError, match="no CPU fallback"):
        fsmn.fsmn_memory(torch.zeros(1, 4, 3), torch.zeros(3, 2), torch.zeros(3, 1))


def test_workspace_size_and_plan_without_a_device():
    lib = _capi.load()
    for name in fm.case_names():
        B, T, D, (lorder, rorder, _, _), _ = fm.CASES[name]
        assert lib.wekws_hip_fsmn_memory_workspace_bytes(B, T, D, lorder, rorder) == fr.workspace_bytes(B, T, D, lorder, rorder), name
    assert fr.workspace_bytes(256, 100, 128, 10, 2) == 256 * 12 * 128 * 8
    assert fr.workspace_bytes(1, 129, 3, 1, 1) % 16 == 0
    # 64-bit sizes: 2^20 rows of 129 frames, 4096 channels, 32 taps -> 2^41 bytes
    assert lib.wekws_hip_fsmn_memory_workspace_bytes(1 << 20, 129, 4096, 20, 12) == (1 << 21) * 32 * 4096 * 8
    for bad in ((0, 5, 4, 3, 1), (2, 0, 4, 3, 1), (2, 5, 0, 3, 1), (2, 5, 4, 0, 1), (2, 5, 4, 3, 0), (-1, 5, 4, 3, 1), (2, 5, 4, 30, 3)):
        assert lib.wekws_hip_fsmn_memory_workspace_bytes(*bad) == 0 and _capi.last_error() != "", bad
    taps = fr.taps(10, 2, 1, 1)
    assert len(taps) == 13 and taps[0] == (fr.SKIP, 0, 2) and taps[1] == (fr.LEFT, 0, 11) and taps[10] == (fr.LEFT, 9, 2)
    assert taps[11] == (fr.RIGHT, 0, 1) and taps[12] == (fr.RIGHT, 1, 0) and fr.window(10, 2, 1, 1) == 12
    assert all(d >= 0 for _, _, d in fr.taps(4, 3, 2, 3)) and fr.window(4, 3, 2, 3) == 16


def test_every_refusal_holds_without_a_device():
    """Argument errors return EINVAL with a message before any launch: nothing here needs (or touches) a device, so the
    pointers are host addresses that are never dereferenced."""
    lib = _capi.load()
    buf = np.zeros(4096, np.float64)
    p = buf.ctypes.data
    assert p % 16 == 0
    ws_bytes = fr.workspace_bytes(2, 5, 4, 3, 1)

    def fwd(x=p, B=2, T=5, D=4, wl=p, lo=3, ls=1, wr=p, ro=1, rs=1, y=p):
        return lib.wekws_hip_fsmn_memory_forward(x, B, T, D, wl, lo, ls, wr, ro, rs, y, None)

    def bwd(x=p, g=p, B=2, T=5, D=4, wl=p, lo=3, ls=1, wr=p, ro=1, rs=1, dx=p, dwl=p, dwr=p, ws=p, nb=ws_bytes):
        return lib.wekws_hip_fsmn_memory_backward(x, g, B, T, D, wl, lo, ls, wr, ro, rs, dx, dwl, dwr, ws, nb, None)

    shape_errors = [dict(B=0), dict(T=0), dict(D=0), dict(B=-3), dict(lo=0), dict(ro=0), dict(ls=0), dict(rs=0), dict(ls=-1),
                    dict(lo=30, ro=3), dict(lo=17, ro=16), dict(lo=10, ro=2, ls=30), dict(lo=2, ro=2, rs=128), dict(lo=4, ro=3, ls=64, rs=22)]
    for call, nulls in ((fwd, ("x", "wl", "wr", "y")), (bwd, ("x", "g", "wl", "wr"))):
        for k in nulls:
            assert call(**{k: None}) == -1 and "NULL" in _capi.last_error(), k
        for kw in shape_errors:
            assert call(**kw) == -1 and _capi.last_error() != "", kw
    assert "taps" in (fwd(lo=30, ro=3), _capi.last_error())[1] and "window" in (fwd(lo=10, ro=2, ls=30), _capi.last_error())[1]
    # a window of exactly 256 frames is inside the limits: refused for nothing but the missing workspace here
    assert bwd(lo=10, ro=3, ls=28, rs=1, ws=None) == -1 and "workspace" in _capi.last_error()
    assert bwd(nb=ws_bytes - 1) == -1 and "workspace" in _capi.last_error()
    assert bwd(nb=0) == -1 and bwd(ws=None) == -1
    assert bwd(ws=p + 8) == -1 and "aligned" in _capi.last_error()
    assert bwd(dwr=None) == -1 and "together" in _capi.last_error()
    assert bwd(dwl=None) == -1 and "together" in _capi.last_error()
    assert not buf.any()
