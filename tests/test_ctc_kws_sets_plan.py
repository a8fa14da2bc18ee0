"""CPU: the keyword-set table of the CTC decoder (wekws_amd/csrc/ctc_kws_sets.h), without a device.

The table decides every refusal of wekws_hip_ctc_kws_add_set / _drop_set / _assign, hands out the set ids and lays out the
device tables.  The hooks library runs a script of operations on it (wekws_hip_debug_ctc_kws_sets) and returns every
operation's outcome and the table's image; both are held to a plain Python model of the registry."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from wekws_amd import _capi

HOOKS = os.path.join(os.path.dirname(_capi.lib_path()), "libwekws_hip_hooks.so")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["add_set", "drop_set", "assign", "stream_set", "search_sets"]


@pytest.fixture(scope="module")
def hooks():
    lib = C.CDLL(HOOKS)
    lib.wekws_hip_debug_ctc_kws_sets.restype = C.c_int
    lib.wekws_hip_debug_ctc_kws_sets.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                                 C.c_int64, C.c_void_p]
    return lib


# ------------------------------------------------------------------------------------------ the script and the image
def add(kws, ts=None, thr=0.5, offsets=None):
    """An add operation; `offsets` overrides the offsets the keywords imply (to state a broken set)."""
    return ("add", [tuple(k) for k in kws], None if ts is None else list(ts), float(thr), offsets)


def encode(ops):
    out = []
    for op in ops:
        if op[0] == "add":
            _, kws, ts, thr, offsets = op
            toks = [t for k in kws for t in k]
            offs = offsets if offsets is not None else [0] + list(np.cumsum([len(k) for k in kws]))
            lo, hi = struct.unpack("<ii", struct.pack("<d", thr))
            out += [0, len(kws), len(toks)] + [int(o) for o in offs] + toks + ([-1] if ts is None else [len(ts)] + ts) + [lo, hi]
        elif op[0] == "drop":
            out += [1, op[1]]
        else:
            out += [2, len(op[1])] + list(op[1]) + list(op[2])
    return np.array(out, np.int32)


def run(hooks, V, n_streams, ops):
    """(outcomes, raw image)"""
    script = encode(ops)
    outcomes = np.full(len(ops), -99, np.int32)
    n = C.c_int64(0)
    assert hooks.wekws_hip_debug_ctc_kws_sets(V, n_streams, script.ctypes.data, script.size, outcomes.ctypes.data, len(ops), None, 0,
                                              C.byref(n)) == len(ops)
    img = np.zeros(n.value, np.int32)
    again = np.full(len(ops), -99, np.int32)
    assert hooks.wekws_hip_debug_ctc_kws_sets(V, n_streams, script.ctypes.data, script.size, again.ctypes.data, len(ops),
                                              img.ctypes.data, img.size, C.byref(n)) == len(ops)
    assert n.value == img.size and again.tolist() == outcomes.tolist()
    return outcomes.tolist(), img


def parse(img, V):
    n_ids, n_kw, n_mask, n_streams = (int(v) for v in img[:4])
    assert img.size == 4 + 7 * n_ids + n_kw + n_mask + n_streams
    recs = img[4:4 + 7 * n_ids].reshape(n_ids, 7)
    kw = img[4 + 7 * n_ids:4 + 7 * n_ids + n_kw]
    mask = img[4 + 7 * n_ids + n_kw:4 + 7 * n_ids + n_kw + n_mask].view(np.uint32)
    stream_set = img[img.size - n_streams:].tolist()
    W = (V + 31) // 32
    sets = {}
    for i, (live, users, base, nk, mw, lo, hi) in enumerate(recs.tolist()):
        if not live:
            continue
        offs = kw[base:base + nk + 1].tolist()
        toks = kw[base + nk + 1:base + nk + 1 + offs[-1]].tolist()
        bits = None
        if mw >= 0:
            assert mw % W == 0 and mw + W <= n_mask
            bits = {s for s in range(W * 32) if (int(mask[mw + (s >> 5)]) >> (s & 31)) & 1}
        sets[i] = dict(users=users, keywords=[tuple(toks[a:b]) for a, b in zip(offs, offs[1:])], tokenset=bits,
                       threshold=struct.pack("<ii", lo, hi), kw_range=(base, base + nk + 1 + offs[-1]), mask_word=mw,
                       first_offset=offs[0])
    return dict(n_ids=n_ids, sets=sets, stream_set=stream_set, W=W)


# ------------------------------------------------------------------------------------------ the model
class Model:
    """The registry as the issue states it: nothing about arenas."""

    def __init__(self, V, n_streams):
        self.V, self.sets, self.stream_set, self.high = V, {}, [0] * n_streams, 0

    def apply(self, op):
        if op[0] == "add":
            _, kws, ts, thr, offsets = op
            toks = [t for k in kws for t in k]
            offs = offsets if offsets is not None else [0] + list(np.cumsum([len(k) for k in kws]))
            if kws and (offs[0] != 0 or any(b <= a for a, b in zip(offs, offs[1:]))):
                return -1
            if any(t < 0 or t >= self.V for t in toks[:offs[-1] if kws else 0]):
                return -1
            if ts is not None and any(t < 0 or t >= self.V for t in ts):
                return -1
            i = 0
            while i in self.sets:
                i += 1
            self.sets[i] = dict(keywords=kws, tokenset=None if ts is None else set(ts), threshold=struct.pack("<d", thr))
            self.high = max(self.high, i + 1)
            return i
        if op[0] == "drop":
            s = op[1]
            if s == 0 or s not in self.sets or s in self.stream_set:
                return -1
            del self.sets[s]
            return 0
        _, ids, sets = op
        if len(set(ids)) != len(ids) or any(i < 0 or i >= len(self.stream_set) for i in ids) or any(s not in self.sets for s in sets):
            return -1
        for i, s in zip(ids, sets):
            self.stream_set[i] = s
        return 0


def check_image(img, model):
    t = parse(img, model.V)
    assert t["n_ids"] == model.high and sorted(t["sets"]) == sorted(model.sets) and t["stream_set"] == model.stream_set
    for i, m in model.sets.items():
        s = t["sets"][i]
        assert s["first_offset"] == 0 and s["keywords"] == m["keywords"] and s["tokenset"] == m["tokenset"]
        assert s["threshold"] == m["threshold"]
        assert s["users"] == model.stream_set.count(i)
    # no two live sets share a word of either arena
    spans = sorted(s["kw_range"] for s in t["sets"].values())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    words = [s["mask_word"] for s in t["sets"].values() if s["mask_word"] >= 0]
    assert len(set(words)) == len(words)
    return t


# ------------------------------------------------------------------------------------------ tests
def test_symbols_are_exported_and_bound_and_the_debug_entry_is_the_hooks_librarys_alone(hooks):
    lib = _capi.load()
    for n in NEW:
        assert hasattr(lib, "wekws_hip_ctc_kws_" + n) and "wekws_hip_ctc_kws_" + n in _capi.SIGNATURES
    src = open(os.path.join(ROOT, "include", "wekws_hip.h")).read()
    assert "#define WEKWS_HIP_ABI_VERSION 2" in src and "wekws_hip_debug" not in src
    assert hasattr(hooks, "wekws_hip_debug_ctc_kws_sets") and not hasattr(lib, "wekws_hip_debug_ctc_kws_sets")
    for n in NEW:
        assert hasattr(hooks, "wekws_hip_ctc_kws_" + n)


def test_every_entry_point_refuses_a_null_handle():
    lib = _capi.load()
    out = C.c_int32(7)
    one = np.zeros(1, np.int32)
    assert lib.wekws_hip_ctc_kws_add_set(None, None, None, 0, None, 0, 0.5, C.byref(out), None) == -1
    assert "NULL" in _capi.last_error() and out.value == 7
    assert lib.wekws_hip_ctc_kws_drop_set(None, 1, None) == -1
    assert lib.wekws_hip_ctc_kws_assign(None, one.ctypes.data, one.ctypes.data, 1, None) == -1
    assert lib.wekws_hip_ctc_kws_stream_set(None, 0) == -1
    assert lib.wekws_hip_ctc_kws_search_sets(None, None, 1, 1, None, None, None, None, None) == -1


def test_ids_start_at_one_and_the_lowest_free_id_is_reused(hooks):
    ops = [add([(1, 2)]), add([(3,)]), add([(4, 5, 6)], ts=[0, 4]), add([]), ("drop", 3), ("drop", 1), add([(7,)]), add([(8,)]),
           add([(9,)])]
    got, img = run(hooks, 33, 4, ops)
    assert got == [0, 1, 2, 3, 0, 0, 1, 3, 4]
    m = Model(33, 4)
    assert [m.apply(o) for o in ops] == got
    t = check_image(img, m)
    assert t["sets"][1]["keywords"] == [(7,)] and t["sets"][3]["keywords"] == [(8,)] and t["sets"][0]["users"] == 4


BASE = [add([(1, 2), (3,)], thr=0.25), add([(4, 5)], ts=[0, 4, 5, 32], thr=0.5), add([(6,)], thr=0.75),
        ("assign", [0, 2], [1, 1]), ("assign", [3], [2])]
REFUSED = {
    "drop_in_use": ("drop", 1),
    "drop_set_0": ("drop", 0),
    "drop_unknown": ("drop", 9),
    "drop_negative": ("drop", -1),
    "empty_keyword": add([(1,), (2,)], offsets=[0, 1, 1]),
    "offsets_decrease": add([(1, 2), (3,)], offsets=[0, 2, 1]),
    "first_offset_not_0": add([(1, 2)], offsets=[1, 2]),
    "token_at_vocab": add([(1, 33)]),
    "token_negative": add([(-1,)]),
    "mask_entry_at_vocab": add([(1,)], ts=[0, 33]),
    "mask_entry_negative": add([(1,)], ts=[-2]),
    "assign_unknown_set": ("assign", [1], [5]),
    "assign_dropped_range_set": ("assign", [1], [-1]),
    "assign_repeated_stream": ("assign", [1, 4, 1], [0, 0, 0]),
    "assign_stream_past_the_end": ("assign", [6], [0]),
    "assign_negative_stream": ("assign", [-1], [0]),
    "assign_good_then_bad": ("assign", [4, 5, 6], [2, 2, 2]),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_a_refused_operation_leaves_the_image_byte_identical(hooks, name):
    V, n = 33, 6
    want, img = run(hooks, V, n, BASE)
    assert want == [0, 1, 2, 0, 0]
    got, img2 = run(hooks, V, n, BASE + [REFUSED[name]])
    assert got == want + [-1]
    assert img2.tobytes() == img.tobytes()
    # ... and what follows behaves as if it had not been tried
    tail = [("assign", [0, 2], [0, 0]), ("drop", 1), add([(7, 8)], ts=[7])]
    a, ia = run(hooks, V, n, BASE + tail)
    b, ib = run(hooks, V, n, BASE + [REFUSED[name]] + tail)
    assert a == [0, 1, 2, 0, 0, 0, 0, 1] and b == a[:5] + [-1] + a[5:] and ia.tobytes() == ib.tobytes()


def random_keywords(rng, V):
    return [tuple(int(x) for x in rng.integers(0, V, int(rng.integers(1, 6)))) for _ in range(int(rng.integers(0, 5)))]


@pytest.mark.parametrize("V", [33, 2599])
@pytest.mark.parametrize("seed", range(3))
def test_random_script_against_the_model(hooks, V, seed):
    rng = np.random.default_rng(1000 * seed + V)
    n = 12
    m = Model(V, n)
    ops = [add([(1, 2)], thr=0.1)]
    want = [m.apply(ops[0])]
    for _ in range(400):
        r = rng.random()
        live = sorted(m.sets) or [0]
        if r < .4:
            kws = random_keywords(rng, V)
            toks = sorted({t for k in kws for t in k})
            ts = None if rng.random() < .3 else sorted({0, V - 1, 31, 32} | set(toks[:int(rng.integers(0, 8))]))
            op = add(kws, ts, float(rng.uniform(0, 1)))
            bad = rng.random()
            if bad < .05 and kws:
                op = add(kws[:-1] + [kws[-1] + (V,)], ts, .5)
            elif bad < .1 and ts is not None:
                op = add(kws, ts + [V + int(rng.integers(0, 40))], .5)
            elif bad < .15 and len(kws) > 1:
                offs = [0] + list(np.cumsum([len(k) for k in kws]))
                offs[1] = offs[2]
                op = add(kws, ts, .5, offsets=offs)
        elif r < .65:
            op = ("drop", int(rng.choice(live + [0, len(live) + 3])) if rng.random() < .3 else int(rng.choice(live)))
        else:
            ids = rng.permutation(n)[:int(rng.integers(0, 6))].tolist()
            if rng.random() < .1 and ids:
                ids = ids + [ids[0]]
            if rng.random() < .1:
                ids = ids + [n + int(rng.integers(0, 3))]
            sets = [int(rng.choice(live)) for _ in ids]
            if rng.random() < .1 and sets:
                sets[-1] = max(live) + 1 + int(rng.integers(0, 3))
            op = ("assign", ids, sets)
        ops.append(op)
        want.append(m.apply(op))
    # two masked sets at the end: a mask at a non-zero word offset whatever the script dropped
    ops += [add([(1,)], ts=[0, 1, 31, 32, V - 1]), add([(2,)], ts=[2, 32])]
    want += [m.apply(ops[-2]), m.apply(ops[-1])]
    got, img = run(hooks, V, n, ops)
    assert got == want
    assert any(o == -1 for o in got[:-2]) and sum(o >= 0 for o in got) > 100
    t = check_image(img, m)
    assert any(s["mask_word"] > 0 for s in t["sets"].values())
    if V == 2599:
        assert t["W"] == 82
    assert any(s["tokenset"] is not None and {31, 32} <= s["tokenset"] for s in t["sets"].values())


def test_a_script_that_does_not_parse_is_refused(hooks):
    n = C.c_int64(0)
    out = np.zeros(4, np.int32)
    for script in ([3], [0, 1, 1, 0, 5, 1, -1, 0, 0], [1], [2, 3, 0], [0, 1]):
        s = np.array(script, np.int32)
        assert hooks.wekws_hip_debug_ctc_kws_sets(33, 2, s.ctypes.data, s.size, out.ctypes.data, 4, None, 0, C.byref(n)) == -1


def test_add_keywords_needs_the_vocabulary():
    from wekws_amd import ctc
    sp = ctc.StreamingKeywordSpotter(2, [(1,)], .5, device="cuda:0")
    with pytest.raises(ValueError, match="vocab="):
        sp.add_keywords([(2, 3)])
    assert sp.keywords_of(1) == 0
    with pytest.raises(ValueError):
        sp.assign([0], 4)
    with pytest.raises(ValueError):
        sp.drop_keywords(0)


def test_a_null_token_set_means_none_whatever_its_length(hooks):
    """token_set NULL is "no first-beam set" for the descriptor and for add_set alike; its length is then not read."""
    lo, hi = struct.unpack("<ii", struct.pack("<d", 0.5))
    script = np.array([0, 1, 2, 0, 2, 1, 2, -1, lo, hi,           # set 0
                       0, 1, 1, 0, 1, 5, -4, lo, hi,              # a NULL token set with token_set_len = 3
                       0, 0, 0, 0, -8, lo, hi], np.int32)         # ... and one of length 7, without keywords
    out = np.full(3, -99, np.int32)
    n = C.c_int64(0)
    assert hooks.wekws_hip_debug_ctc_kws_sets(33, 2, script.ctypes.data, script.size, out.ctypes.data, 3, None, 0, C.byref(n)) == 3
    img = np.zeros(n.value, np.int32)
    assert hooks.wekws_hip_debug_ctc_kws_sets(33, 2, script.ctypes.data, script.size, out.ctypes.data, 3, img.ctypes.data, img.size,
                                              C.byref(n)) == 3
    assert out.tolist() == [0, 1, 2]
    t = parse(img, 33)
    assert [t["sets"][i]["tokenset"] for i in range(3)] == [None, None, None]
    assert t["sets"][1]["keywords"] == [(5,)] and t["sets"][2]["keywords"] == []
    # the descriptor: create gets past its validation (to the device, where there is one)
    import torch
    lib = _capi.load()
    flat, offs = np.array([1, 2], np.int32), np.array([0, 2], np.int32)
    d = _capi.CtcKwsDesc(vocab=33, score_beam=3, path_beam=20, num_keywords=1, keyword_tokens=flat.ctypes.data,
                         keyword_offsets=offs.ctypes.data, token_set=None, token_set_len=3, downsampling=1, max_streams=1,
                         prefix_capacity=8, device=0, threshold=0.5)
    h = C.c_void_p()
    rc = lib.wekws_hip_ctc_kws_create(C.byref(d), C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h, _capi.last_error()
        lib.wekws_hip_ctc_kws_destroy(h)
    else:
        assert rc == -3 and not h, (rc, _capi.last_error())
