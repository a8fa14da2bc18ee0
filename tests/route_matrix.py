"""The route matrix: conv-model calls at the edges where the routing of wekws_amd/csrc/route.h changes its choice, each with the
route of every tile PREDICTED here and confirmed twice:
  * on the CPU (tests/test_route.py): every prediction equals what route.h's select_conv_route returns for the call
    (wekws_hip_debug_conv_route of the hooks library), and the rows reach every (family, nt, ctx, fast, split, persistent) tuple a
    sweep of the recipes and of the fuzz generator reaches -- a route.h change that adds a variant fails until a row is added;
  * on the GPU (tests/test_hip_route_matrix.py): the tile trace of the real forward (wekws_hip_debug_route_trace) equals the
    prediction, and every chunk's output and the final cache meet the tight bar against the float64 oracle.

A row: the model (a synth.MODEL_CONFIGS name, with overrides for shape variants), precision and options, B, the chunk sequence
(the cache carried from chunk to chunk), an incoming cache (random and nonzero: a zero cache hides hand-over bugs) or none, and
feature / cache offsets in floats (1: pointers only 4-byte aligned, made by slicing one float into a larger buffer).  EXPECT holds
per chunk the route of every tile: "family nt ctx fast pers upw split", pers = fewer workgroups than utterances (a persistent
grid), upw = utterances per workgroup.  The predictions assume CUS compute units (MI355X); the GPU test checks the device has them.
"""
import copy
import ctypes as C
import math
import os

import numpy as np

from wekws_amd import _capi, pack
from wekws_amd.utils import synth

CUS = 256
TILE = 112                     # WEKWS_HIP_TILE_FRAMES
FAMILIES = ["none", "ds256_stream", "ds256_g32", "ds256_mm", "ds256_g16", "ds256_w16", "ds64_g4", "mdtc64_stream", "mdtc64_g4",
            "mdtc64_w16", "mdtc32_g4", "dense_stack_f16", "conv_stack_f16", "conv_stack"]
KEYS = ("plan", "C", "ks", "family", "nt", "split", "ctx", "fast", "grid", "threads", "lds", "utts_per_wg", "cache_len", "max_pad", "head_slices",
        "eff")
TRACE_KEYS = ("family", "nt", "split", "ctx", "fast", "grid", "threads", "lds", "utts_per_wg")


def hooks_path():
    return os.path.join(os.path.dirname(_capi.lib_path()), "libwekws_hip_hooks.so")


def type_hooks(lib):
    lib.wekws_hip_debug_conv_route.restype = C.c_int
    lib.wekws_hip_debug_conv_route.argtypes = [C.POINTER(_capi.Desc), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                               C.c_char_p, C.c_int]
    lib.wekws_hip_debug_route_trace.restype = C.c_int
    lib.wekws_hip_debug_route_trace.argtypes = [C.POINTER(C.c_int), C.c_int]
    for f in (lib.wekws_hip_debug_gru_route, lib.wekws_hip_debug_fsmn_route):
        f.restype = C.c_int
        f.argtypes = [C.POINTER(_capi.Desc), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    return lib


def route(lib, cfg, B, T, has_in=False, has_out=True, precision="default", x16=1, cache16=1, cus=CUS, ntiles=1, opts=None):
    """route.h's choice for one tile, on the CPU (wekws_hip_debug_conv_route)."""
    cfg = dict(cfg)
    cfg["_precision"] = precision
    d = _capi.make_desc(dict(pack.parse_config(cfg), abi_version=_capi.ABI_VERSION))
    call = (C.c_int * 8)(B, T, ntiles, int(has_in), int(has_out), x16, cache16, cus)
    out = (C.c_int * len(KEYS))()
    why = C.create_string_buffer(256)
    o = (C.c_int * 9)(*opts) if opts is not None else None
    assert lib.wekws_hip_debug_conv_route(C.byref(d), o, call, out, why, 256) == 0
    r = dict(zip(KEYS, list(out)))
    r["family"] = FAMILIES[r["family"]]
    r["plan"] = ["as_is", "padded", "generic"][r["plan"]]
    r["eff"] = PRECISIONS[r["eff"]]
    r["why"] = why.value.decode()
    return r


PLANS = ["as_is", "padded", "generic"]
PRECISIONS = ["default", "f32", "f16x3", "f16"]                 # enum wekws_hip_precision
GRU_FAMILIES = ["none", "gru_f32", "gru_f16", "gru_pipe"]
# the 9 ints of a GRU trace record (wekws_hip_hooks.hip: route_record), then what only the CPU entry point reports
GRU_REC = ("family", "nn", "spw", "tchunk", "nchunks", "slots", "tiles", "grid", "bits")
GRU_KEYS = ("plan", "C") + GRU_REC + ("stages", "slots_p", "lds", "chunked", "plain", "gran", "res_plain", "res_gran", "eff")
FSMN_REC = ("tile_frames", "nt", "u", "head_slices", "grid", "lds", "ntiles", "_0", "_1")
FSMN_KEYS = ("plan", "max_nt") + FSMN_REC + ("ws", "eff")


def _desc(cfg, precision):
    cfg = dict(cfg)
    cfg["_precision"] = precision
    return _capi.make_desc(dict(pack.parse_config(cfg), abi_version=_capi.ABI_VERSION))


def _opts(opts):
    pairs = [v for k, val in (opts or {}).items() for v in (_capi.OPTIONS[k], int(val))]
    return (C.c_int * max(1, len(pairs)))(*pairs), len(pairs) // 2


def gru_route(lib, cfg, B, T, precision="default", x16=1, cus=CUS, reserve=False, opts=None):
    """route.h's choice for one GRU call, on the CPU (wekws_hip_debug_gru_route); opts: {option name: value}."""
    d = _desc(cfg, precision)
    o, n = _opts(opts)
    out = (C.c_int64 * 20)()
    why = C.create_string_buffer(256)
    assert lib.wekws_hip_debug_gru_route(C.byref(d), o, n, (C.c_int * 5)(B, T, x16, cus, int(reserve)), out, why, 256) == 0
    r = dict(zip(GRU_KEYS, list(out)))
    r.update(plan=PLANS[r["plan"]], family=GRU_FAMILIES[r["family"]], eff=PRECISIONS[r["eff"]], why=why.value.decode())
    r.update(pk=r["bits"] & 1, k2=(r["bits"] >> 1) & 1, nf_in_kernel=(r["bits"] >> 2) & 1)
    return r


def fsmn_route(lib, cfg, B, T, tile=0, precision="default", cus=CUS, opts=None):
    """route.h's choice for tile `tile` of one FSMN call, on the CPU (wekws_hip_debug_fsmn_route)."""
    d = _desc(cfg, precision)
    o, n = _opts(opts)
    out = (C.c_int64 * 16)()
    why = C.create_string_buffer(256)
    assert lib.wekws_hip_debug_fsmn_route(C.byref(d), o, n, (C.c_int * 4)(B, T, tile, cus), out, why, 256) == 0
    r = dict(zip(FSMN_KEYS, list(out)))
    r.update(plan=PLANS[r["plan"]], eff=PRECISIONS[r["eff"]], why=why.value.decode())
    return r


def gru_record(r):
    return [r[k] for k in GRU_REC]


def fsmn_record(r):
    return [r[k] for k in FSMN_REC]


# GRU and FSMN calls of the recipes (tools/bench_configs.py): batches of 98 frames (FSMN-CTC: 32 / 64 spliced frames) and
# 10-frame streaming chunks.  tests/test_route.py pins route.h's routes for them; tests/test_hip_route_gru_fsmn.py checks that the
# forward's trace on the device is that route.
GRU_CALLS = [("gru_2x128", B, T) for B, T in ((1, 10), (1, 98), (256, 10), (256, 98), (1024, 98), (16384, 98))]
FSMN_CALLS = [("fsmn_ctc", B, T) for B, T in ((1, 10), (256, 10), (1024, 32), (1024, 64), (4096, 32))]


def route_str(r, B):
    """'family nt ctx fast pers upw split' of a route (from route() or a trace record)."""
    pers = int(r["grid"] * r["utts_per_wg"] < B)
    return f"{r['family']} nt{r['nt']} ctx{r['ctx']} fast{r['fast']} pers{pers} upw{r['utts_per_wg']} split{r['split']}"


def route_tuple(s):
    """(family, nt, ctx, fast, split, persistent) of a route string."""
    f, nt, ctx, fast, pers, _, split = s.split()
    return (f, int(nt[2:]), int(ctx[3:]), int(fast[4:]), int(split[5:]), int(pers[4:]))


def _r(id, model, chunks, B=1, precision="default", opts=None, over=None, cache=False, x_off=0, c_off=0):
    return dict(id=id, model=model, over=over or {}, precision=precision, opts=opts or {}, B=B, chunks=list(chunks), cache=cache,
                x_off=x_off, c_off=c_off)


def _rows():
    S = []
    r = lambda *a, **k: S.append(_r(*a, **k))                                         # noqa: E731
    Q = [(1, 16), (17, 32), (33, 64), (65, 112)]          # the nt boundaries: 1 / 2 / 4 / 7 tiles of 16 frames, first and later chunk
    # DS-TCN h256
    for a, b in Q:
        r(f"ds256/default/B1/{a}+{b}", "ds_tcn_h256", (a, b), B=1 if a < 65 else 3)
    for a, b in Q:
        r(f"ds256/nostream/B3/{a}+{b}", "ds_tcn_h256", (a, b), B=3, opts={"stream": 0})
    for a, b in Q:
        r(f"ds256/x16_0/B3/{a}+{b}", "ds_tcn_h256", (a, b), B=3, opts={"stream": 0}, x_off=1)
    for a, b in Q:
        r(f"ds256/g16_off/B2/{a}+{b}", "ds_tcn_h256", (a, b), B=2, opts={"g16": 0, "stream": 0})
    for a, b in Q:
        r(f"ds256/f32/B3/{a}+{b}", "ds_tcn_h256", (a, b), B=3, precision="f32")
    for a, b in Q:
        r(f"ds256/f32_x16_0/B1/{a}+{b}", "ds_tcn_h256", (a, b), B=1, precision="f32", x_off=1)
    for a, b in Q:
        r(f"ds256/persistent/B{CUS + 1}/{a}+{b}", "ds_tcn_h256", (a, b), B=CUS + 1, opts={"stream": 0})
    r(f"ds256/persistent/B{CUS - 1}/65+40", "ds_tcn_h256", (65, 40), B=CUS - 1)
    r(f"ds256/persistent/B{CUS}/65+40", "ds_tcn_h256", (65, 40), B=CUS)
    r(f"ds256/persistent/B{2 * CUS + 1}/33+17", "ds_tcn_h256", (33, 17), B=2 * CUS + 1)
    for T in (1, 17, 33, 65):
        r(f"ds256/f32_persistent/B{CUS + 1}/{T}", "ds_tcn_h256", (T,), B=CUS + 1, precision="f32")
    r(f"ds256/f32_persistent/B{2 * CUS + 1}/40", "ds_tcn_h256", (40,), B=2 * CUS + 1, precision="f32")
    r("ds256/T113", "ds_tcn_h256", (113,), B=2)
    r("ds256/T225_cache", "ds_tcn_h256", (225,), B=2, cache=True)
    r("ds256/f32_T225_cache", "ds_tcn_h256", (225,), B=1, precision="f32", cache=True)
    r("ds256/cache16_0/T10", "ds_tcn_h256", (10, 10), B=3, cache=True, c_off=1)
    r("ds256/stream_cache/T10x3", "ds_tcn_h256", (10, 10, 10), B=5, cache=True)
    # CTC-sized heads: the matrix-core kernel, head slices on small calls
    for a, b in Q[:3]:
        r(f"ds256_ctc300/B1/{a}+{b}", "ds_tcn_h256_ctc300", (a, b), B=1)
    r("ds256_ctc2599/B2/65+112", "ds_tcn_h256_ctc", (65, 112), B=2)
    r("ds256_ctc300/T150_cache", "ds_tcn_h256_ctc300", (150,), B=1, cache=True)
    # DS-TCN h64
    for a, b in Q:
        r(f"ds64/default/B3/{a}+{b}", "ds_tcn_h64", (a, b), B=3)
    for a, b in Q:
        r(f"ds64/x16_0/B3/{a}+{b}", "ds_tcn_h64", (a, b), B=3, x_off=1)
    r("ds64/T225_cache", "ds_tcn_h64", (225,), B=1, cache=True)
    # plain TCN
    for a, b in Q:
        r(f"tcn64/default/B1/{a}+{b}", "tcn_h64", (a, b), B=1)
    r("tcn64/f32/B3/40+40", "tcn_h64", (40, 40), B=3, precision="f32")
    # MDTC h64
    for a, b in Q:
        r(f"mdtc64/default/B3/{a}+{b}", "mdtc_h64", (a, b), B=3)
    for a, b in Q:
        r(f"mdtc64/x16_0/B1/{a}+{b}", "mdtc_h64", (a, b), B=1, x_off=1)
    r("mdtc64/nostream/B3/1+16", "mdtc_h64", (1, 16), B=3, opts={"stream": 0})
    r("mdtc64/cache16_0/T10", "mdtc_h64", (10, 10), B=3, cache=True, c_off=1)
    r("mdtc64/T113_cache", "mdtc_h64", (113,), B=3, cache=True)
    r("mdtc64/f32/B3/17+65", "mdtc_h64", (17, 65), B=3, precision="f32")
    r("mdtc64_global12/B3/40+40", "mdtc_h64_global12", (40, 40), B=3)
    # MDTC h32
    for a, b in Q:
        r(f"mdtc32/default/B3/{a}+{b}", "mdtc_small", (a, b), B=3)
    for a, b in Q:
        r(f"mdtc32/x16_0/B5/{a}+{b}", "mdtc_small", (a, b), B=5, x_off=1)
    # shapes without a kernel of their own: zero-padded widths and the any-shape path
    r("padded/ds_h200/B3/33+17", "ds_tcn_h256", (33, 17), B=3, over={"hidden_dim": 200})
    r("padded/tcn_h48_k5/B3/40+40", "tcn_h64", (40, 40), B=3, over={"hidden_dim": 48, "backbone.kernel_size": 5})
    r("padded/mdtc_h48/B3/17+10", "mdtc_h64", (17, 10), B=3, over={"hidden_dim": 48, "backbone.hidden_dim": 48})
    r("generic/ds_h320/B2/40+20", "ds_tcn_h64", (40, 20), B=2, over={"hidden_dim": 320})
    r("generic/mdtc_k7/B2/30+30", "mdtc_small", (30, 30), B=2, over={"backbone.kernel_size": 7})
    return S


ROWS = _rows()


def row_config(row):
    cfg = copy.deepcopy(synth.MODEL_CONFIGS[row["model"]])
    for k, v in row["over"].items():
        if k.startswith("backbone."):
            cfg["backbone"][k.split(".", 1)[1]] = v
        else:
            cfg[k] = v
    cfg["_precision"] = row["precision"]
    return cfg


def row_weights(row, cfg):
    return synth.synth_state_dict(pack.model_spec(cfg), 1234 + ROWS.index(row))


def row_input(row, cfg):
    return synth.synth_feats(row["B"], sum(row["chunks"]), cfg["input_dim"], seed=7 + ROWS.index(row))


def row_cache(row, cfg):
    """The incoming cache: random and nonzero, or None."""
    if not row["cache"]:
        return None
    shape = pack.cache_shape(pack.parse_config(cfg), row["B"])
    return (0.5 * np.random.default_rng([0xCA, ROWS.index(row)]).standard_normal(shape)).astype(np.float32)


def route_opts(row, precision=None):
    """The options array of wekws_hip_debug_conv_route for the row's options (the product defaults otherwise)."""
    p = precision or row["precision"]
    o = row["opts"]
    g16 = o.get("g16", 1)
    return [o.get("w16", 1), int(g16 != 0), int(g16 != 3), int(g16 == 2), o.get("stream", 1), o.get("mdtc16", 1), o.get("mm", -1),
            int(p == "f32"), int(p != "f16")]


def predict(lib, row, precision=None):
    """(plan, [per chunk: [route string of every tile]]) from route.h, for the calls the row's forward makes."""
    p = precision or row["precision"]
    cfg = row_config(row)
    idim = cfg["input_dim"]
    first = route(lib, cfg, row["B"], 1, precision=p)
    plan = first["plan"]
    if plan == "generic":
        return plan, [[] for _ in row["chunks"]]
    out = []
    for j, T in enumerate(row["chunks"]):
        has_in = row["cache"] or j > 0
        ntiles = math.ceil(T / TILE)
        x16 = int(row["x_off"] % 4 == 0 and (T * idim) % 4 == 0)
        # (widened models hand the kernels aligned copies of the caller's caches: aux_kernels.hip's cache_remap_kernel)
        cache16 = int(plan == "padded" or not (has_in and row["c_off"] % 4))
        tiles = []
        for i in range(ntiles):
            Tt = min(TILE, T - i * TILE)
            r = route(lib, cfg, row["B"], Tt, has_in=has_in or i > 0, has_out=True, precision=p, x16=x16, cache16=cache16, ntiles=ntiles,
                      opts=route_opts(row, p))
            assert r["plan"] == plan
            tiles.append(route_str(r, row["B"]))
        out.append(tiles)
    return plan, out


# the families with a one-fp16-product variant (precision F16); the others run three products (or exact f32) whatever is asked
ONE_PRODUCT = ("ds256_stream", "ds256_g16", "ds256_w16", "ds64_g4", "mdtc64_stream", "mdtc64_g4", "mdtc64_w16", "mdtc32_g4")


def is_split_row(row):
    """F16X3 rows (neither exact f32 nor the any-shape path): the ones the F16 negative control reruns."""
    return row["precision"] != "f32" and EXPECT[row["id"]][0] != "generic"


# Predicted routes, per row id: (plan, per chunk [route of every tile]).  tests/test_route.py checks them against route.h.
EXPECT = {
    'ds256/default/B1/1+16': ('as_is', [
        ['ds256_stream nt1 ctx1 fast0 pers0 upw1 split1'],
        ['ds256_stream nt1 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/default/B1/17+32': ('as_is', [
        ['ds256_g16 nt2 ctx0 fast1 pers0 upw1 split1'],
        ['ds256_g16 nt4 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'ds256/default/B1/33+64': ('as_is', [
        ['ds256_g16 nt4 ctx0 fast1 pers0 upw1 split1'],
        ['ds256_g16 nt4 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'ds256/default/B1/65+112': ('as_is', [
        ['ds256_g16 nt7 ctx0 fast1 pers0 upw1 split1'],
        ['ds256_g16 nt7 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'ds256/nostream/B3/1+16': ('as_is', [
        ['ds256_g16 nt1 ctx0 fast1 pers0 upw1 split1'],
        ['ds256_w16 nt1 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/nostream/B3/17+32': ('as_is', [
        ['ds256_g16 nt2 ctx0 fast1 pers0 upw1 split1'],
        ['ds256_g16 nt4 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'ds256/nostream/B3/33+64': ('as_is', [
        ['ds256_g16 nt4 ctx0 fast1 pers0 upw1 split1'],
        ['ds256_g16 nt4 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'ds256/nostream/B3/65+112': ('as_is', [
        ['ds256_g16 nt7 ctx0 fast1 pers0 upw1 split1'],
        ['ds256_g16 nt7 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'ds256/x16_0/B3/1+16': ('as_is', [
        ['ds256_g16 nt1 ctx0 fast0 pers0 upw1 split1'],
        ['ds256_w16 nt1 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/x16_0/B3/17+32': ('as_is', [
        ['ds256_g16 nt2 ctx0 fast0 pers0 upw1 split1'],
        ['ds256_w16 nt2 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/x16_0/B3/33+64': ('as_is', [
        ['ds256_g16 nt4 ctx0 fast0 pers0 upw1 split1'],
        ['ds256_w16 nt4 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/x16_0/B3/65+112': ('as_is', [
        ['ds256_g16 nt7 ctx0 fast0 pers0 upw1 split1'],
        ['ds256_w16 nt7 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/g16_off/B2/1+16': ('as_is', [
        ['ds256_w16 nt1 ctx0 fast0 pers0 upw1 split1'],
        ['ds256_w16 nt1 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/g16_off/B2/17+32': ('as_is', [
        ['ds256_w16 nt2 ctx0 fast0 pers0 upw1 split1'],
        ['ds256_w16 nt2 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/g16_off/B2/33+64': ('as_is', [
        ['ds256_w16 nt4 ctx0 fast0 pers0 upw1 split1'],
        ['ds256_w16 nt4 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/g16_off/B2/65+112': ('as_is', [
        ['ds256_w16 nt7 ctx0 fast0 pers0 upw1 split1'],
        ['ds256_w16 nt7 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/f32/B3/1+16': ('as_is', [
        ['ds256_g32 nt1 ctx0 fast1 pers0 upw1 split1'],
        ['conv_stack nt1 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/f32/B3/17+32': ('as_is', [
        ['ds256_g32 nt2 ctx0 fast1 pers0 upw1 split1'],
        ['conv_stack nt2 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/f32/B3/33+64': ('as_is', [
        ['ds256_g32 nt4 ctx0 fast1 pers0 upw1 split1'],
        ['conv_stack nt4 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/f32/B3/65+112': ('as_is', [
        ['ds256_g32 nt7 ctx0 fast1 pers0 upw1 split1'],
        ['conv_stack nt7 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/f32_x16_0/B1/1+16': ('as_is', [
        ['conv_stack nt1 ctx0 fast0 pers0 upw1 split1'],
        ['conv_stack nt1 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/f32_x16_0/B1/17+32': ('as_is', [
        ['conv_stack nt2 ctx0 fast0 pers0 upw1 split1'],
        ['conv_stack nt2 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/f32_x16_0/B1/33+64': ('as_is', [
        ['conv_stack nt4 ctx0 fast0 pers0 upw1 split1'],
        ['conv_stack nt4 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/f32_x16_0/B1/65+112': ('as_is', [
        ['conv_stack nt7 ctx0 fast0 pers0 upw1 split1'],
        ['conv_stack nt7 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/persistent/B257/1+16': ('as_is', [
        ['ds256_g16 nt1 ctx0 fast1 pers1 upw1 split1'],
        ['ds256_w16 nt1 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/persistent/B257/17+32': ('as_is', [
        ['ds256_g16 nt2 ctx0 fast1 pers1 upw1 split1'],
        ['ds256_g16 nt4 ctx1 fast1 pers1 upw1 split1'],
    ]),
    'ds256/persistent/B257/33+64': ('as_is', [
        ['ds256_g16 nt4 ctx0 fast1 pers1 upw1 split1'],
        ['ds256_g16 nt4 ctx1 fast1 pers1 upw1 split1'],
    ]),
    'ds256/persistent/B257/65+112': ('as_is', [
        ['ds256_g16 nt7 ctx0 fast1 pers1 upw1 split1'],
        ['ds256_g16 nt7 ctx1 fast1 pers1 upw1 split1'],
    ]),
    'ds256/persistent/B255/65+40': ('as_is', [
        ['ds256_g16 nt7 ctx0 fast1 pers0 upw1 split1'],
        ['ds256_g16 nt4 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'ds256/persistent/B256/65+40': ('as_is', [
        ['ds256_g16 nt7 ctx0 fast1 pers0 upw1 split1'],
        ['ds256_g16 nt4 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'ds256/persistent/B513/33+17': ('as_is', [
        ['ds256_g16 nt4 ctx0 fast1 pers1 upw1 split1'],
        ['ds256_g16 nt4 ctx1 fast1 pers1 upw1 split1'],
    ]),
    'ds256/f32_persistent/B257/1': ('as_is', [
        ['ds256_g32 nt1 ctx0 fast1 pers1 upw1 split1'],
    ]),
    'ds256/f32_persistent/B257/17': ('as_is', [
        ['ds256_g32 nt2 ctx0 fast1 pers1 upw1 split1'],
    ]),
    'ds256/f32_persistent/B257/33': ('as_is', [
        ['ds256_g32 nt4 ctx0 fast1 pers1 upw1 split1'],
    ]),
    'ds256/f32_persistent/B257/65': ('as_is', [
        ['ds256_g32 nt7 ctx0 fast1 pers1 upw1 split1'],
    ]),
    'ds256/f32_persistent/B513/40': ('as_is', [
        ['ds256_g32 nt4 ctx0 fast1 pers1 upw1 split1'],
    ]),
    'ds256/T113': ('as_is', [
        ['ds256_g16 nt7 ctx0 fast1 pers0 upw1 split1', 'ds256_w16 nt1 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/T225_cache': ('as_is', [
        ['ds256_g16 nt7 ctx1 fast1 pers0 upw1 split1', 'ds256_g16 nt7 ctx1 fast1 pers0 upw1 split1', 'ds256_w16 nt1 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/f32_T225_cache': ('as_is', [
        ['conv_stack nt7 ctx1 fast0 pers0 upw1 split1', 'conv_stack nt7 ctx1 fast0 pers0 upw1 split1', 'conv_stack nt1 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/cache16_0/T10': ('as_is', [
        ['ds256_w16 nt1 ctx1 fast0 pers0 upw1 split1'],
        ['ds256_w16 nt1 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256/stream_cache/T10x3': ('as_is', [
        ['ds256_stream nt1 ctx1 fast0 pers0 upw1 split1'],
        ['ds256_stream nt1 ctx1 fast0 pers0 upw1 split1'],
        ['ds256_stream nt1 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256_ctc300/B1/1+16': ('as_is', [
        ['ds256_mm nt1 ctx0 fast0 pers0 upw1 split1'],
        ['ds256_mm nt1 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256_ctc300/B1/17+32': ('as_is', [
        ['ds256_mm nt2 ctx0 fast0 pers0 upw1 split1'],
        ['ds256_mm nt2 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256_ctc300/B1/33+64': ('as_is', [
        ['ds256_mm nt4 ctx0 fast0 pers0 upw1 split1'],
        ['ds256_mm nt4 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256_ctc2599/B2/65+112': ('as_is', [
        ['ds256_mm nt7 ctx0 fast0 pers0 upw1 split1'],
        ['ds256_mm nt7 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds256_ctc300/T150_cache': ('as_is', [
        ['ds256_mm nt7 ctx1 fast0 pers0 upw1 split1', 'ds256_mm nt4 ctx1 fast0 pers0 upw1 split1'],
    ]),
    'ds64/default/B3/1+16': ('as_is', [
        ['ds64_g4 nt1 ctx0 fast1 pers0 upw1 split1'],
        ['conv_stack_f16 nt1 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'ds64/default/B3/17+32': ('as_is', [
        ['ds64_g4 nt2 ctx0 fast1 pers0 upw1 split1'],
        ['ds64_g4 nt4 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'ds64/default/B3/33+64': ('as_is', [
        ['ds64_g4 nt4 ctx0 fast1 pers0 upw1 split1'],
        ['ds64_g4 nt4 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'ds64/default/B3/65+112': ('as_is', [
        ['ds64_g4 nt7 ctx0 fast1 pers0 upw1 split1'],
        ['ds64_g4 nt7 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'ds64/x16_0/B3/1+16': ('as_is', [
        ['conv_stack_f16 nt1 ctx0 fast0 pers0 upw2 split1'],
        ['conv_stack_f16 nt1 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'ds64/x16_0/B3/17+32': ('as_is', [
        ['conv_stack_f16 nt2 ctx0 fast0 pers0 upw2 split1'],
        ['conv_stack_f16 nt2 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'ds64/x16_0/B3/33+64': ('as_is', [
        ['conv_stack_f16 nt4 ctx0 fast0 pers0 upw2 split1'],
        ['conv_stack_f16 nt4 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'ds64/x16_0/B3/65+112': ('as_is', [
        ['conv_stack_f16 nt7 ctx0 fast0 pers0 upw2 split1'],
        ['conv_stack_f16 nt7 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'ds64/T225_cache': ('as_is', [
        ['ds64_g4 nt7 ctx1 fast1 pers0 upw1 split1', 'ds64_g4 nt7 ctx1 fast1 pers0 upw1 split1', 'conv_stack_f16 nt1 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'tcn64/default/B1/1+16': ('as_is', [
        ['dense_stack_f16 nt1 ctx0 fast0 pers0 upw2 split1'],
        ['dense_stack_f16 nt1 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'tcn64/default/B1/17+32': ('as_is', [
        ['dense_stack_f16 nt2 ctx0 fast0 pers0 upw2 split1'],
        ['dense_stack_f16 nt2 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'tcn64/default/B1/33+64': ('as_is', [
        ['dense_stack_f16 nt4 ctx0 fast0 pers0 upw2 split1'],
        ['dense_stack_f16 nt4 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'tcn64/default/B1/65+112': ('as_is', [
        ['dense_stack_f16 nt7 ctx0 fast0 pers0 upw2 split1'],
        ['dense_stack_f16 nt7 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'tcn64/f32/B3/40+40': ('as_is', [
        ['conv_stack nt4 ctx0 fast0 pers0 upw2 split1'],
        ['conv_stack nt4 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'mdtc64/default/B3/1+16': ('as_is', [
        ['mdtc64_stream nt1 ctx1 fast0 pers0 upw2 split1'],
        ['mdtc64_stream nt1 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'mdtc64/default/B3/17+32': ('as_is', [
        ['mdtc64_g4 nt2 ctx0 fast1 pers0 upw1 split1'],
        ['mdtc64_g4 nt4 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'mdtc64/default/B3/33+64': ('as_is', [
        ['mdtc64_g4 nt4 ctx0 fast1 pers0 upw1 split1'],
        ['mdtc64_g4 nt4 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'mdtc64/default/B3/65+112': ('as_is', [
        ['mdtc64_g4 nt7 ctx0 fast1 pers0 upw1 split1'],
        ['mdtc64_g4 nt7 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'mdtc64/x16_0/B1/1+16': ('as_is', [
        ['mdtc64_w16 nt1 ctx0 fast0 pers0 upw2 split1'],
        ['mdtc64_w16 nt1 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'mdtc64/x16_0/B1/17+32': ('as_is', [
        ['mdtc64_w16 nt2 ctx0 fast0 pers0 upw2 split1'],
        ['mdtc64_w16 nt2 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'mdtc64/x16_0/B1/33+64': ('as_is', [
        ['mdtc64_w16 nt4 ctx0 fast0 pers0 upw2 split1'],
        ['mdtc64_w16 nt4 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'mdtc64/x16_0/B1/65+112': ('as_is', [
        ['mdtc64_w16 nt7 ctx0 fast0 pers0 upw2 split1'],
        ['mdtc64_w16 nt7 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'mdtc64/nostream/B3/1+16': ('as_is', [
        ['mdtc64_g4 nt1 ctx0 fast1 pers0 upw1 split1'],
        ['mdtc64_w16 nt1 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'mdtc64/cache16_0/T10': ('as_is', [
        ['mdtc64_w16 nt1 ctx1 fast0 pers0 upw2 split1'],
        ['mdtc64_w16 nt1 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'mdtc64/T113_cache': ('as_is', [
        ['mdtc64_g4 nt7 ctx1 fast1 pers0 upw1 split1', 'mdtc64_w16 nt1 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'mdtc64/f32/B3/17+65': ('as_is', [
        ['conv_stack nt2 ctx0 fast0 pers0 upw2 split1'],
        ['conv_stack nt7 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'mdtc64_global12/B3/40+40': ('as_is', [
        ['mdtc64_g4 nt4 ctx0 fast1 pers0 upw1 split1'],
        ['mdtc64_w16 nt4 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'mdtc32/default/B3/1+16': ('as_is', [
        ['mdtc32_g4 nt1 ctx0 fast1 pers0 upw1 split1'],
        ['conv_stack_f16 nt1 ctx1 fast0 pers0 upw4 split1'],
    ]),
    'mdtc32/default/B3/17+32': ('as_is', [
        ['mdtc32_g4 nt2 ctx0 fast1 pers0 upw1 split1'],
        ['mdtc32_g4 nt4 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'mdtc32/default/B3/33+64': ('as_is', [
        ['mdtc32_g4 nt4 ctx0 fast1 pers0 upw1 split1'],
        ['mdtc32_g4 nt4 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'mdtc32/default/B3/65+112': ('as_is', [
        ['mdtc32_g4 nt7 ctx0 fast1 pers0 upw1 split1'],
        ['mdtc32_g4 nt7 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'mdtc32/x16_0/B5/1+16': ('as_is', [
        ['conv_stack_f16 nt1 ctx0 fast0 pers0 upw4 split1'],
        ['conv_stack_f16 nt1 ctx1 fast0 pers0 upw4 split1'],
    ]),
    'mdtc32/x16_0/B5/17+32': ('as_is', [
        ['conv_stack_f16 nt2 ctx0 fast0 pers0 upw4 split1'],
        ['conv_stack_f16 nt2 ctx1 fast0 pers0 upw4 split1'],
    ]),
    'mdtc32/x16_0/B5/33+64': ('as_is', [
        ['conv_stack_f16 nt4 ctx0 fast0 pers0 upw4 split1'],
        ['conv_stack_f16 nt4 ctx1 fast0 pers0 upw4 split1'],
    ]),
    'mdtc32/x16_0/B5/65+112': ('as_is', [
        ['conv_stack_f16 nt7 ctx0 fast0 pers0 upw4 split1'],
        ['conv_stack_f16 nt7 ctx1 fast0 pers0 upw4 split1'],
    ]),
    'padded/ds_h200/B3/33+17': ('padded', [
        ['ds256_g16 nt4 ctx0 fast1 pers0 upw1 split1'],
        ['ds256_g16 nt4 ctx1 fast1 pers0 upw1 split1'],
    ]),
    'padded/tcn_h48_k5/B3/40+40': ('padded', [
        ['dense_stack_f16 nt4 ctx0 fast0 pers0 upw2 split1'],
        ['dense_stack_f16 nt4 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'padded/mdtc_h48/B3/17+10': ('padded', [
        ['mdtc64_g4 nt2 ctx0 fast1 pers0 upw1 split1'],
        ['mdtc64_stream nt1 ctx1 fast0 pers0 upw2 split1'],
    ]),
    'generic/ds_h320/B2/40+20': ('generic', [
        [],
        [],
    ]),
    'generic/mdtc_k7/B2/30+30': ('generic', [
        [],
        [],
    ]),
}
