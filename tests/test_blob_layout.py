"""CPU: the layout of the weight blob (wekws_amd/csrc/blob_layout.h) against the packer (wekws_amd/pack.py), WITHOUT a GPU, through
the hooks library: wekws_hip_debug_blob_layout gives the tensors in blob order (offset, rows, cols, inner), wekws_hip_debug_blob_tensor
one tensor by the name of the accessor the library's own code reads it with.  Every model of synth.MODEL_CONFIGS, and per backbone one
shape that runs zero-padded and one that runs on the any-shape path (the overrides of tests/route_matrix.py / route_matrix_rnn.py rows;
FSMN is never padded, and no matrix row puts a plain TCN on the any-shape path: it takes the DS-TCN row's width), and the heads
that no synth model pairs with a backbone."""
import ctypes as C

import pytest

from tests import route_matrix as rm
from tests import route_matrix_rnn as rr
from wekws_amd import _capi, pack
from wekws_amd.utils import synth

MAX_TENSORS = 256


def _row(mod, rid):
    return next(r for r in mod.ROWS if r["id"] == rid)


VARIANTS = {name: dict(model=name, over={}, precision="default") for name in synth.MODEL_CONFIGS}
VARIANTS.update({
    "padded/ds_tcn": _row(rm, "padded/ds_h200/B3/33+17"),
    "padded/tcn": _row(rm, "padded/tcn_h48_k5/B3/40+40"),
    "padded/mdtc": _row(rm, "padded/mdtc_h48/B3/17+10"),
    "padded/gru": _row(rr, "gru/f16/padded_h64/B7/T10x2"),
    "generic/ds_tcn": _row(rm, "generic/ds_h320/B2/40+20"),
    "generic/tcn": dict(model="tcn_h64", over=_row(rm, "generic/ds_h320/B2/40+20")["over"], precision="default"),
    "generic/mdtc": _row(rm, "generic/mdtc_k7/B2/30+30"),
    "generic/gru": _row(rr, "gru/any_shape/h160/B2/T17"),
    "generic/fsmn": _row(rr, "fsmn/any_shape/small_lo40/B2/T30_cache"),
    # heads no synth model gives these backbones (the head's tensors lie behind the units whatever the backbone)
    "heads/tcn_global": dict(model="tcn_h64", over={"classifier": {"type": "global", "dropout": 0.5}}, precision="default"),
    "heads/ds_tcn_last": dict(model="ds_tcn_h64", over={"classifier": {"type": "last", "dropout": 0.5}}, precision="default"),
    "heads/ds_tcn_identity": dict(model="ds_tcn_h64", over={"classifier": {"type": "identity"}, "output_dim": 64}, precision="default"),
    "heads/gru_global": dict(model="gru_2x128", over={"classifier": {"type": "global", "dropout": 0.5}}, precision="default"),
})


@pytest.fixture(scope="module")
def hooks():
    lib = C.CDLL(rm.hooks_path())
    lib.wekws_hip_debug_blob_layout.restype = C.c_int
    lib.wekws_hip_debug_blob_layout.argtypes = [C.POINTER(_capi.Desc), C.POINTER(C.c_int64), C.c_int]
    lib.wekws_hip_debug_blob_tensor.restype = C.c_int
    lib.wekws_hip_debug_blob_tensor.argtypes = [C.POINTER(_capi.Desc), C.c_char_p, C.c_int, C.POINTER(C.c_int64)]
    lib.wekws_hip_blob_elems.restype = C.c_size_t
    lib.wekws_hip_blob_elems.argtypes = [C.POINTER(_capi.Desc)]
    return lib


def case(variant):
    """(descriptor dict, [(name, folded tensor)] of the packer) of a variant."""
    cfg = rm.row_config(VARIANTS[variant])
    d, parts = pack._parts(cfg, synth.synth_state_dict(pack.model_spec(cfg), 1))
    return {k: int(d[k]) for k in pack.DESC_FIELDS}, parts


def enumeration(lib, desc):
    """[(offset, rows, cols, inner)] of the blob's tensors, in blob order."""
    out = (C.c_int64 * (4 * MAX_TENSORS))()
    n = lib.wekws_hip_debug_blob_layout(C.byref(_capi.make_desc(desc)), out, MAX_TENSORS)
    assert 0 < n <= MAX_TENSORS, (n, _capi.last_error())
    return [tuple(out[4 * i:4 * i + 4]) for i in range(n)]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_enumeration_is_the_packers_blob(hooks, variant):
    desc, parts = case(variant)
    tensors = enumeration(hooks, desc)
    # contiguous from 0, and ends where both statements of the size say the blob ends
    at = 0
    for off, rows, cols, inner in tensors:
        assert off == at and rows > 0 and cols > 0 and inner > 0, (variant, tensors)
        at += rows * cols * inner
    assert at == hooks.wekws_hip_blob_elems(C.byref(_capi.make_desc(desc))) == pack.blob_elems(desc)
    # tensor by tensor the packer's parts: element counts and (rows, cols x inner)
    assert [r * c * i for _, r, c, i in tensors] == [p.size for _, p in parts]
    assert [(r, c * i) for _, r, c, i in tensors] == [p.reshape(p.shape[0], -1).shape for _, p in parts]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_accessors_name_the_packers_tensors(hooks, variant):
    """Neighbours of equal size (W1 / W2 of an MDTC block, W_ih / W_hh of a GRU layer) cannot be told apart by size: the tensor an
    accessor NAMES is the enumeration's tensor at the position where the packer puts the part of that name."""
    desc, parts = case(variant)
    tensors = enumeration(hooks, desc)
    d = _capi.make_desc(desc)
    names = [n for n, _ in parts]
    out = (C.c_int64 * 4)()
    for k, name in enumerate(names):
        unit = names[:k].count(name)                              # the packer repeats a name once per block / layer
        assert hooks.wekws_hip_debug_blob_tensor(C.byref(d), name.encode(), unit, out) == 0, name
        assert tuple(out) == tensors[k], (variant, k, name, unit)
    if desc["backbone"] in (pack.BACKBONE["mdtc"], pack.BACKBONE["gru"]):
        a, b = ("w1", "w2") if desc["backbone"] == pack.BACKBONE["mdtc"] else ("w_ih", "w_hh")
        ia, ib = names.index(a), names.index(b)
        assert ia < ib and tensors[ia][1:] == tensors[ib][1:] and tensors[ia][0] < tensors[ib][0]
    # a tensor the model does not have has no elements (among the names of its own backbone: the sections' slots are shared); a
    # name that does not exist is refused
    if desc["backbone"] in (pack.BACKBONE["ds_tcn"], pack.BACKBONE["tcn"], pack.BACKBONE["mdtc"]):
        for name in sorted({"wd", "bd", "w2", "b2", "head_w2", "head_b2"} - set(names)):
            assert hooks.wekws_hip_debug_blob_tensor(C.byref(d), name.encode(), 0, out) == 0 and out[1] * out[2] * out[3] == 0, name
    assert hooks.wekws_hip_debug_blob_tensor(C.byref(d), b"w3", 0, out) == -1


def test_enumerations_differ_where_the_descriptors_differ(hooks):
    """(the hook does not return a constant) Two variants have the same enumeration exactly when their descriptors agree in what
    the layout depends on: every size, the backbone, and whether the head is none, one matrix or two."""
    def key(desc):
        two = desc["head"] in (pack.HEAD["glob"], pack.HEAD["last"])
        return tuple(desc[k] for k in pack.DESC_FIELDS if k not in ("head", "activation", "precision", "preproc_relu")) + (
            desc["head"] == pack.HEAD["identity"], two)
    seen = {}
    for variant in sorted(VARIANTS):
        desc, _ = case(variant)
        seen.setdefault(key(desc), set()).add(tuple(enumeration(hooks, desc)))
    assert all(len(v) == 1 for v in seen.values())
    assert len({next(iter(v)) for v in seen.values()}) == len(seen) > len(VARIANTS) // 2


def test_an_invalid_descriptor_has_no_layout(hooks):
    desc, _ = case("ds_tcn_h64")
    out = (C.c_int64 * 4)()
    assert hooks.wekws_hip_debug_blob_layout(C.byref(_capi.make_desc({**desc, "num_layers": 0})), out, 1) == -1
    assert hooks.wekws_hip_debug_blob_layout(None, out, 1) == -1
