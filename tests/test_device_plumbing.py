"""wekws_amd._device without a device: the module walk every ``use_device_*`` swap is made of, and the float32 check every
layer's entry point opens with.  The six callers are covered by their own test_*_modules.py."""
import pytest
import torch
import torch.nn as nn

from wekws_amd import _device


class _Twin(nn.Identity):
    pass


def test_swap_children_replaces_what_is_wanted_once():
    keep_outer, keep_inner = nn.ReLU(), nn.Linear(3, 3)
    a, b, c = nn.Tanh(), nn.Tanh(), nn.Tanh()
    net = nn.Sequential(a, keep_outer, nn.Sequential(b, keep_inner, nn.Sequential(c)))
    made = {}

    def make(child):
        made[child] = _Twin()
        return made[child]

    assert _device.swap_children(net, lambda m: isinstance(m, nn.Tanh), make) == 3
    assert set(made) == {a, b, c}
    assert net[0] is made[a] and net[2][0] is made[b] and net[2][2][0] is made[c]          # nested children are reached
    assert net[1] is keep_outer and net[2][1] is keep_inner
    assert not any(isinstance(m, nn.Tanh) for m in net.modules())
    # the replacements are not wanted: nothing is made, nothing moves
    assert _device.swap_children(net, lambda m: isinstance(m, nn.Tanh), make) == 0
    assert len(made) == 3 and net[0] is made[a]


def test_swap_children_does_not_revisit_a_replacement():
    net = nn.Sequential(nn.Sequential(nn.Tanh()), nn.Tanh())
    # every replacement is itself wanted and has a wanted child: the walk is over a snapshot, so neither is seen (the three
    # are the two children of `net` and the child of the inner container as it was)
    assert _device.swap_children(net, lambda m: isinstance(m, (nn.Tanh, nn.Sequential)), lambda m: nn.Sequential(nn.Tanh())) == 3


# Without a device every tensor here is a CPU tensor: "float64" is refused as one before its dtype is looked at (the dtype alone is
# tests/test_hip_device_plumbing.py's), and the second text, "tensors on one device", needs two devices and is not raised here.
@pytest.mark.parametrize("bad", [torch.zeros(2), torch.zeros(2, dtype=torch.float64), None, [1.0]], ids=["cpu", "float64", "none", "list"])
def test_require_float32_names_the_offending_argument(bad):
    with pytest.raises(ValueError) as err:
        _device.require_float32("some_op", bad, (("weight", bad),))
    assert str(err.value) == "some_op: weight must be a float32 tensor on a ROCm device (no CPU fallback)"
