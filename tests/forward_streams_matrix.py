"""The case table of wekws_hip_forward_streams: every table-driven kernel instance and every reason for the grouped path, as data.
No torch import: the CPU test (tests/test_forward_streams_plan.py) asks route.h's plan_streams for the plan of every case and holds
it to the `expect` written here; the GPU child (tests/tools/forward_streams_matrix_cases.py) runs the same cases on the device and
tests/test_hip_forward_streams_matrix.py judges what it measured.

A case: the model (a synth.MODEL_CONFIGS name plus overrides, named as in tests/route_matrix.py / route_matrix_rnn.py), the
precision, Tcap, B = B[0] x CUs + B[1], the frame counts (frames_of), softmax or not, and the expected plan: kind, then (nt, u) for
fsmn_f16, the split for ds256_stream, the reason for grouped.  `device_only` marks the one reason that plan_streams is TOLD by its
caller (the pool's plane size is no multiple of 4 floats) and the CPU entry point therefore cannot see."""
import copy
import ctypes as C

import numpy as np

from tests import route_matrix as rm
from wekws_amd import _capi
from wekws_amd.utils import synth

CUS = 256
SENTINEL = 777.0
EDGES = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)      # the edges of the FSMN kernel's 16-frame tiles
PADDED = "a zero-padded model or the any-shape path"
WHY_DS_TILE = "rows longer than ds256_stream's tile of 16 frames"
WHY_FSMN_TILE = "rows longer than the FSMN kernel's tile"
WHY_NO_CONV = "no table-driven kernel for this conv model"
WHY_GRU = "no table-driven GRU kernel"


KINDS = ["grouped", "ds256_stream", "fsmn_f16"]


def type_plan(lib):
    """The hooks library, typed for plan(): rm.type_hooks plus wekws_hip_debug_streams_plan."""
    lib = rm.type_hooks(lib)
    lib.wekws_hip_debug_streams_plan.restype = C.c_int
    lib.wekws_hip_debug_streams_plan.argtypes = [C.POINTER(_capi.Desc), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_void_p,
                                                 C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return lib


def plan(lib, cfg, Tcap, frames, cus=CUS, opts=None):
    """route.h's plan_streams for one call, without a device (wekws_hip_debug_streams_plan); the precision is cfg's _precision."""
    d = rm._desc(cfg, cfg.get("_precision", "default"))
    o, n = rm._opts(opts)
    B = len(frames)
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    order, start, gT = np.full(B, -7, np.int32), np.full(B + 1, -7, np.int32), np.full(B, -7, np.int32)
    out = (C.c_int * 16)()
    why = C.create_string_buffer(256)
    assert lib.wekws_hip_debug_streams_plan(C.byref(d), o, n, (C.c_int * 3)(B, Tcap, cus), fr.ctypes.data, out, order.ctypes.data,
                                            start.ctypes.data, gT.ctypes.data, why, 256) == 0
    keys = ("kind", "live", "max_T", "ngroups", "slots", "family", "split", "conv_grid", "conv_lds", "nt", "u", "head_slices", "fsmn_grid",
            "fsmn_lds")
    p = dict(zip(keys, list(out)))
    p["kind"] = KINDS[p["kind"]]
    p["why"] = why.value.decode()
    p["order"] = order[:p["live"]].tolist()
    p["groups"] = [(int(gT[g]), order[start[g]:start[g + 1]].tolist()) for g in range(p["ngroups"])]
    return p


def case_config(case):
    cfg = copy.deepcopy(synth.MODEL_CONFIGS[case["model"]])
    for k, v in case["over"].items():
        if k.startswith("backbone."):
            cfg["backbone"][k.split(".", 1)[1]] = v
        else:
            cfg[k] = v
    cfg["_precision"] = case["precision"]
    return cfg


def rows_of(case, cus=CUS):
    return case["B"][0] * cus + case["B"][1]


# ---------------------------------------------------------------------------------------------------------------------------------
# a. the FSMN instances: one call each.  `frames`: ("list", counts) for the small calls, ("packed", cap, single) for the packed ones.
def _fsmn(id, model, Tcap, B, frames, nt, u, softmax=False):
    return dict(id="fsmn/" + id, group="a", model=model, over={}, precision="default", Tcap=Tcap, B=B, frames=frames, softmax=softmax,
                expect=dict(kind="fsmn_f16", nt=nt, u=u))


def packed_counts(B, Tcap, u, single):
    """B frame counts for a packed instance: one row with 0 frames, one with -1, ONE row at `single` (a group with one live slot),
    the other rows over the remaining tile edges up to Tcap -- Tcap among them -- so that some count's rows are no multiple of u.  Only
    two rows are skipped: the instance is chosen from the LIVE rows, and B is just above u x CUs."""
    others = [e for e in EDGES if e <= Tcap and e != single]
    n = B - 3
    counts = [n // len(others) + (1 if i < n % len(others) else 0) for i in range(len(others))]
    if all(c % u == 0 for c in counts):
        counts[0] += 1
        counts[-1] -= 1
    fr = [0, -1, single] + [e for e, c in zip(others, counts) for _ in range(c)]
    assert len(fr) == B and Tcap in fr and any(c % u for c in counts)
    return fr


def frames_of(case, cus=CUS):
    """(stream ids, frame counts) of a one-call case: the counts in a fixed permutation, the ids a permutation of the pool's
    streams (the pool holds two more than the call has rows: they are left out)."""
    B = rows_of(case, cus)
    kind = case["frames"][0]
    rng = np.random.default_rng(B * 131 + case["Tcap"])
    if kind == "list":
        fr = list(case["frames"][1])
    else:
        fr = [int(v) for v in rng.permutation(packed_counts(B, case["Tcap"], case["expect"]["u"], case["frames"][1]))]
    assert len(fr) == B
    ids = [int(v) for v in rng.permutation(B + 2)[:B]]
    return ids, fr


FSMN_CASES = [
    _fsmn("nt1_u1", "fsmn_small", 16, (0, 5), ("list", [16, 0, 1, -1, 15]), 1, 1),
    _fsmn("nt2_u1", "fsmn_small", 32, (0, 5), ("list", [32, 0, 17, -1, 1]), 2, 1),
    _fsmn("nt3_u1", "fsmn_small", 48, (0, 5), ("list", [16, 48, -1, 33, 0]), 3, 1),
    _fsmn("nt4_u1", "fsmn_small", 64, (0, 5), ("list", [0, 49, 15, 64, -1]), 4, 1),
    _fsmn("nt1_u2", "fsmn_small", 16, (2, 3), ("packed", 15), 1, 2),
    _fsmn("nt2_u2", "fsmn_small", 32, (2, 3), ("packed", 31), 2, 2),
    _fsmn("nt1_u4", "fsmn_small", 16, (4, 3), ("packed", 15), 1, 4),
    # the instance follows the largest LIVE count, not Tcap: nt = 2 over rows whose stride is 64 frames
    _fsmn("nt2_stride64", "fsmn_small", 64, (0, 7), ("list", [20, 0, 1, 17, -1, 16, 15]), 2, 1),
    # head_slices = 8 at nt = 2, the softmax behind it
    _fsmn("ctc300_nt2_slices", "fsmn_ctc300", 32, (0, 5), ("list", [32, -1, 17, 0, 16]), 2, 1, softmax=True),
]
FSMN_INSTANCES = [(1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (2, 2), (1, 4)]     # the switch of fsmn_f16_rows.hip

# b. ds256_stream's table-driven variants
DS256_CASES = [
    dict(id="ds256/f16", group="b", model="ds_tcn_h256", over={}, precision="f16", Tcap=16, B=(0, 5), frames=("list", [1, 16, 7, 0, 10]),
         softmax=False, expect=dict(kind="ds256_stream", split=0)),
    dict(id="ds256/softmax", group="b", model="ds_tcn_h256", over={}, precision="default", Tcap=16, B=(0, 5),
         frames=("list", [1, 16, 7, 0, 10]), softmax=True, expect=dict(kind="ds256_stream", split=1)),
]

# ---------------------------------------------------------------------------------------------------------------------------------
# c. the grouped path: three calls of 5 rows on a pool of 7 streams.  Ids and resets as in tests/tools/forward_streams_cases.py: a
# stream left out of the middle call (5), streams in all three (6, 3), one that enters late (4), one reset before the third call (0).
STREAMS = 7
SCHEDULE_IDS = [([6, 2, 0, 5, 3], []), ([3, 0, 6, 2, 4], []), ([5, 6, 3, 0, 2], [0])]
FRAMES16 = [[10, 0, 3, 16, 1], [1, 16, 7, -1, 5], [4, 16, 9, 2, 1]]


def _grouped(id, model, Tcap, frames, why, over=None, precision="default", softmax=False, pooled=False, cache_shape=None,
             device_only=False):
    assert len(frames) == 3 and all(len(f) == 5 and max(f) <= Tcap for f in frames)
    return dict(id="grouped/" + id, group="c", model=model, over=over or {}, precision=precision, Tcap=Tcap, B=(0, 5), frames=frames,
                softmax=softmax, pooled=pooled, cache_shape=cache_shape, device_only=device_only, expect=dict(kind="grouped", why=why))


GROUPED_CASES = [
    # rows longer than a tile: the un-skipped 30-frame chunk of DS-TCN h256 (two rows share a count), FSMN tiles chained in a bucket
    _grouped("ds256_T30", "ds_tcn_h256", 30, [[30, 0, 17, 16, 1], [17, 30, 16, -1, 17], [1, 30, 16, 2, 16]], WHY_NO_CONV),
    # (the same stride with no row above ds256_stream's tile: its route is there, Tcap alone refuses it)
    _grouped("ds256_T30_short", "ds_tcn_h256", 30, FRAMES16, WHY_DS_TILE),
    _grouped("ds256_ctc300_softmax", "ds_tcn_h256_ctc300", 16, FRAMES16, WHY_NO_CONV, softmax=True),
    _grouped("fsmn_T80", "fsmn_small", 80, [[80, 0, 65, 64, 3], [3, 80, 64, -1, 65], [64, 80, 3, 65, 64]], WHY_FSMN_TILE),
    _grouped("gru_T40", "gru_2x128", 40, [[40, 0, 17, 16, 1], [1, 40, 7, -1, 33], [4, 40, 9, 2, 40]], WHY_GRU),
    # zero-padded models: the pool holds the caller's narrow geometry
    _grouped("padded_ds_h200", "ds_tcn_h256", 16, FRAMES16, PADDED, over={"hidden_dim": 200}, cache_shape=(1, 200, 105)),
    _grouped("padded_mdtc_h48", "mdtc_h64", 16, FRAMES16, PADDED, over={"hidden_dim": 48, "backbone.hidden_dim": 48}),
    _grouped("padded_gru_h64", "gru_2x128", 16, FRAMES16, PADDED, over={"hidden_dim": 64}, cache_shape=(2, 1, 64)),
    # the any-shape path
    _grouped("generic_ds_h320", "ds_tcn_h64", 16, FRAMES16, PADDED, over={"hidden_dim": 320}),
    _grouped("generic_fsmn_f32", "fsmn_small", 16, FRAMES16, PADDED, precision="f32"),
    # pooled heads: y is (B, odim)
    _grouped("mdtc_small_global12", "mdtc_small_global12", 16, FRAMES16, WHY_NO_CONV, pooled=True),
    _grouped("mdtc_small_last12", "mdtc_small_last12", 16, FRAMES16, WHY_NO_CONV, pooled=True),
    # a per-stream cache of 39 x 5 = 195 floats: no multiple of 4, so the pool's planes are not 16-byte aligned
    _grouped("fsmn_cache195", "fsmn_small", 16, FRAMES16, PADDED, over={"backbone.proj_dim": 39, "backbone.num_layers": 1},
             cache_shape=(1, 39, 5, 1), device_only=True),
]

# e. non-finite input in packed groups: all rows live, counts from the tile edges
NONFINITE_CASES = [
    dict(id="nonfinite/nt1_u2", group="e", model="fsmn_small", over={}, precision="default", Tcap=16, B=(2, 3), softmax=False,
         edges=(1, 7, 16), expect=dict(kind="fsmn_f16", nt=1, u=2)),
    dict(id="nonfinite/nt2_u2", group="e", model="fsmn_small", over={}, precision="default", Tcap=32, B=(2, 3), softmax=False,
         edges=(9, 17, 32), expect=dict(kind="fsmn_f16", nt=2, u=2)),
]


def nonfinite_frames(case, cus=CUS):
    B = rows_of(case, cus)
    rng = np.random.default_rng(B + case["Tcap"])
    return [int(v) for v in rng.permutation(B)], [int(v) for v in rng.permutation(np.resize(case["edges"], B))]


CASES = FSMN_CASES + DS256_CASES + GROUPED_CASES + NONFINITE_CASES
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def plan_calls(case, cus=CUS):
    """The frame-count lists of the case's calls (what plan_streams sees)."""
    if case["group"] == "c":
        return [list(f) for f in case["frames"]]
    if case["group"] == "e":
        return [nonfinite_frames(case, cus)[1]]
    return [frames_of(case, cus)[1]]
