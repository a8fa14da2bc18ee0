"""CPU: the routing layer (wekws_amd/csrc/route.h) -- which shape a conv model runs as (as it is / zero-padded / any-shape path) and
which kernel family serves a call -- swept WITHOUT a GPU through the hooks library's wekws_hip_debug_conv_route.  All three defects
the round-5 fuzz found lived in this layer and needed a GPU to show; their configurations are explicit cases here, and the fuzz
generator's configurations are swept against the invariants of every choice.  The route matrix (tests/route_matrix.py) predicts the
route of every tile of calls at the edges of the choice; here each prediction is checked against route.h, the matrix against every
route a sweep reaches, and the tight parity bar against both sides of its calibration.  (The GPU side -- that wekws_hip_forward takes
exactly the predicted route, and meets the bar there: tests/test_hip_route_matrix.py.)"""
import copy
import ctypes as C

import numpy as np
import pytest

from tests.helpers import random_model_config
from tests.route_matrix import hooks_path, route, type_hooks
from wekws_amd.utils import synth


@pytest.fixture(scope="module")
def hooks():
    return type_hooks(C.CDLL(hooks_path()))


M = synth.MODEL_CONFIGS


@pytest.mark.parametrize("name,kw,family,nt", [
    ("ds_tcn_h256", dict(B=1024, T=98), "ds256_g16", 7),                                   # the headline
    ("ds_tcn_h256", dict(B=1024, T=98, precision="f32"), "ds256_g32", 7),
    ("ds_tcn_h256", dict(B=3, T=80, has_in=True), "ds256_g16", 7),                         # later chunk: the context variant
    ("ds_tcn_h256", dict(B=3, T=20, has_in=True), "ds256_g16", 4),                         # (the context tile is one 16-lane row: >= 4 tiles)
    ("ds_tcn_h256", dict(B=4096, T=10, has_in=True), "ds256_stream", 1),
    ("ds_tcn_h256", dict(B=1, T=10, has_in=False, has_out=True), "ds256_stream", 1),        # first chunk of a stream
    ("ds_tcn_h256", dict(B=1, T=10, has_in=True, cache16=0), "ds256_w16", 1),              # unaligned cache: no 16-byte moves
    ("ds_tcn_h256", dict(B=2, T=98, x16=0), "ds256_g16", 7),                               # unaligned features: its general instantiation
    ("ds_tcn_h256_ctc300", dict(B=2, T=40), "ds256_mm", 4),
    ("ds_tcn_h64", dict(B=1024, T=98), "ds64_g4", 7),
    ("ds_tcn_h64", dict(B=1, T=80, has_in=True), "ds64_g4", 7),
    ("ds_tcn_h64", dict(B=1, T=10, has_in=True), "conv_stack_f16", 1),
    ("ds_tcn_h64", dict(B=8, T=98, precision="f32"), "conv_stack", 7),
    ("tcn_h64", dict(B=8, T=98), "dense_stack_f16", 7),
    ("mdtc_h64", dict(B=1024, T=98), "mdtc64_g4", 7),
    ("mdtc_h64", dict(B=1024, T=10, has_in=True), "mdtc64_stream", 1),
    ("mdtc_h64", dict(B=1, T=98, has_in=True), "mdtc64_w16", 7),                           # one or two streams at 65 .. 112 frames
    ("mdtc_h64", dict(B=3, T=98, has_in=True), "mdtc64_g4", 7),
    ("mdtc_h64_global12", dict(B=8, T=98), "mdtc64_g4", 7),
    ("mdtc_h64_global12", dict(B=8, T=98, has_in=True), "mdtc64_w16", 7),                  # pooled heads with a cache: the LDS-tile kernel
    ("mdtc_small", dict(B=1024, T=98), "mdtc32_g4", 7),
    ("mdtc_small", dict(B=8, T=10, has_in=True), "conv_stack_f16", 1),
])
def test_recipes_take_the_kernel_they_were_built_for(hooks, name, kw, family, nt):
    r = route(hooks, M[name], **kw)
    assert (r["plan"], r["family"], r["nt"]) == ("as_is", family, nt), r


def test_round5_defects_are_visible_without_a_gpu(hooks):
    # (1) DS-TCN h256 with a FIFTH block (dilation 16, padding 112): ds256_w16's hand-over wrote one 64-column pass.  The shape is
    #     outside the register-resident / streaming kernels (dilations 1 / 2 / 4 / 8) and must land on the kernel that walks any padding
    cfg = copy.deepcopy(M["ds_tcn_h256"])
    cfg["backbone"]["num_layers"] = 5
    for kw in (dict(T=98), dict(T=10, has_in=True), dict(T=80, has_in=True)):
        r = route(hooks, cfg, B=3, **kw)
        assert r["family"] == "ds256_w16" and r["max_pad"] == 112, r
    # (2) DS-TCN / TCN with hidden_dim 32 were taken for a built width (32 is built for MDTC only): they run as 64
    for ds in (True, False):
        cfg = copy.deepcopy(M["ds_tcn_h64"])
        cfg["hidden_dim"] = 32
        cfg["backbone"]["ds"] = ds
        r = route(hooks, cfg, B=3, T=50)
        assert (r["plan"], r["C"]) == ("padded", 64) and r["family"] != "none", r
    cfg = copy.deepcopy(M["mdtc_small"])
    assert route(hooks, cfg, B=3, T=50)["plan"] == "as_is"
    # (3) (the empty mel filter was a front-end check: tests/test_hip_fbank.py)


@pytest.mark.parametrize("seed", range(40))
def test_fuzz_configurations_keep_the_invariants_of_every_choice(hooks, seed):
    rng = np.random.default_rng([0x207E, seed])
    seen = set()
    for _ in range(120):
        cfg, head = random_model_config(rng)
        if cfg["backbone"]["type"] == "gru":
            continue
        B = int(rng.choice([1, 2, 3, 9, 260, 1024, 5000]))
        T = int(rng.integers(1, 113))
        has_in = bool(rng.integers(0, 2))
        precision = str(rng.choice(["default", "f32", "f16"]))
        kw = dict(B=B, T=T, has_in=has_in, has_out=bool(rng.integers(0, 2)) or has_in, precision=precision, x16=int(rng.integers(0, 4) > 0),
                  cache16=int(rng.integers(0, 4) > 0), cus=256)
        r = route(hooks, cfg, **kw)
        what = (cfg, kw, r)
        C0, ks0 = cfg["hidden_dim"], cfg["backbone"]["kernel_size"]
        mdtc = cfg["backbone"]["type"] == "mdtc"
        if r["plan"] == "generic":
            assert r["why"], what
            continue
        # the shape the kernels run: a built width that holds the model's, the built kernel size
        assert r["C"] in ((32, 64, 128) if mdtc else (64, 128, 256)) and r["C"] >= C0 and r["ks"] == (5 if mdtc else 8) and ks0 <= r["ks"], what
        assert (r["plan"] == "padded") == (r["C"] != C0 or r["ks"] != ks0), what
        # every shape wekws_hip_create takes has a kernel for every call
        assert r["family"] != "none", what
        assert r["nt"] in (1, 2, 4, 7) and 16 * r["nt"] >= T and 0 < r["lds"] <= 160 * 1024 and r["threads"] in (128, 256, 512, 1024), what
        assert r["grid"] >= 1 and r["grid"] * r["utts_per_wg"] >= min(B, r["grid"] * r["utts_per_wg"]), what
        if r["grid"] * r["utts_per_wg"] < B:                     # fewer workgroups than utterances: a persistent kernel
            assert r["family"] in ("ds256_g16", "ds256_g32") and r["fast"] and r["grid"] == 256, what
        if r["ctx"]:
            assert has_in or r["family"].endswith("stream"), what
        if r["family"].endswith("stream"):
            assert T <= 16 and (has_in or kw["has_out"]) and kw["cache16"] and precision != "f32", what
        if r["family"] in ("ds256_g16", "ds256_g32", "ds64_g4", "mdtc64_g4", "mdtc32_g4", "ds256_stream", "mdtc64_stream"):
            assert r["max_pad"] <= (r["ks"] - 1) * 8, what        # register-resident / streaming kernels: dilations 1 / 2 / 4 / 8
        if r["family"] in ("ds256_g32", "conv_stack"):
            assert precision == "f32", what
        if precision == "f32":
            assert r["family"] in ("ds256_g32", "conv_stack"), what
        if has_in and r["family"] in ("ds256_g16", "ds64_g4", "mdtc64_g4", "mdtc32_g4"):
            assert r["ctx"] and r["nt"] >= 4 and head == "linear", what
        seen.add(r["family"])
    assert len(seen) >= 4


# ---------------------------------------------------------------------------------------------------------------------------------
# the route matrix (tests/route_matrix.py)
from tests import route_matrix as rm  # noqa: E402
from tests.helpers import TIGHT_K, tight_errors  # noqa: E402

ROW_IDS = [r["id"] for r in rm.ROWS]


@pytest.mark.parametrize("row", rm.ROWS, ids=ROW_IDS)
def test_route_matrix_predictions_are_route_h(hooks, row):
    """Every tile's predicted route is what route.h chooses for the call the forward makes; the F16 rerun of a split row says one
    fp16 product (split 0) exactly on the families that have that variant."""
    assert rm.predict(hooks, row) == rm.EXPECT[row["id"]]
    if rm.is_split_row(row):
        _, f16 = rm.predict(hooks, row, "f16")
        for t in (t for ch in f16 for t in ch):
            assert not t.startswith("none") and t.endswith("split0") == (t.split()[0] in rm.ONE_PRODUCT), f16


def _reachable(lib):
    """Every (family, nt, ctx, fast, split, persistent) route.h reaches: the recipes over the calls at the edges of the choice, and
    the fuzz generator's configurations (the sweep of test_fuzz_configurations_keep_the_invariants_of_every_choice)."""
    import itertools
    seen = {}
    conv = [n for n, c in M.items() if c["backbone"]["type"] in ("tcn", "mdtc")]
    cus = rm.CUS
    for name in conv:
        for B, T, hi, ho, p, x16, c16, nti in itertools.product((1, 2, 3, cus - 1, cus, cus + 1, 2 * cus + 1), (1, 16, 17, 32, 33, 64, 65, 112),
                                                              (0, 1), (0, 1), ("default", "f32", "f16"), (0, 1), (0, 1), (1, 2)):
            if nti == 2 and not ho:
                continue
            r = route(lib, M[name], B, T, has_in=hi, has_out=ho, precision=p, x16=x16, cache16=c16, ntiles=nti)
            if r["family"] != "none":
                seen.setdefault(rm.route_tuple(rm.route_str(r, B)), (name, B, T, hi, ho, p, x16, c16, nti))
    for seed in range(40):
        rng = np.random.default_rng([0x207E, seed])
        for _ in range(120):
            cfg, head = random_model_config(rng)
            if cfg["backbone"]["type"] == "gru":
                continue
            B = int(rng.choice([1, 2, 3, 9, 260, 1024, 5000]))
            kw = dict(B=B, T=int(rng.integers(1, 113)), has_in=bool(rng.integers(0, 2)))
            kw.update(has_out=bool(rng.integers(0, 2)) or kw["has_in"], precision=str(rng.choice(["default", "f32", "f16"])),
                      x16=int(rng.integers(0, 4) > 0), cache16=int(rng.integers(0, 4) > 0), cus=256)
            r = route(lib, cfg, **kw)
            if r["family"] != "none":
                seen.setdefault(rm.route_tuple(rm.route_str(r, B)), (cfg, kw))
    return seen


def test_route_matrix_covers_every_reachable_route(hooks):
    """A route.h change that adds a variant fails here until the matrix has a row that runs it on the GPU."""
    have = set()
    for row in rm.ROWS:
        have.update(rm.route_tuple(t) for ch in rm.EXPECT[row["id"]][1] for t in ch)
        if rm.is_split_row(row):                       # (the F16 negative control of the GPU test runs these rows once more)
            have.update(rm.route_tuple(t) for ch in rm.predict(hooks, row, "f16")[1] for t in ch)
    reach = _reachable(hooks)
    missing = {t: reach[t] for t in reach if t not in have}
    assert not missing, missing
    assert len(reach) >= 140
    plans = {rm.EXPECT[r["id"]][0] for r in rm.ROWS}
    assert plans == {"as_is", "padded", "generic"}


def test_route_matrix_rows_cover_the_edges():
    rows = rm.ROWS
    firsts = {r["chunks"][0] for r in rows} | {t for r in rows for t in r["chunks"]}
    assert {1, 16, 17, 32, 33, 64, 65, 112, 113, 225} <= firsts
    assert {rm.CUS - 1, rm.CUS, rm.CUS + 1, 2 * rm.CUS + 1} <= {r["B"] for r in rows}
    assert any(r["B"] == 1 for r in rows)
    upw = [(r["B"], t) for r in rows for ch in rm.EXPECT[r["id"]][1] for t in ch if "upw1" not in t]
    assert any(B % 2 == 1 for B, _ in upw), upw
    assert any(r["x_off"] for r in rows) and any(r["c_off"] and r["cache"] for r in rows)
    assert {"ds_tcn_h256_ctc300", "ds_tcn_h256_ctc"} <= {r["model"] for r in rows}
    assert any(r["cache"] for r in rows) and any(len(r["chunks"]) > 1 for r in rows)


def _calibration_case(row, Bmax=4):
    """The row's model, input (at most Bmax utterances: the bar is per element) and incoming cache."""
    cfg = rm.row_config(row)
    sd = rm.row_weights(row, cfg)
    x = rm.row_input(row, cfg)[:Bmax]
    c0 = rm.row_cache(row, cfg)
    return cfg, sd, x, (None if c0 is None else c0[:Bmax])


@pytest.mark.parametrize("row", rm.ROWS, ids=ROW_IDS)
def test_tight_bar_separates_f32_from_one_fp16_product(row):
    """The tight bar (tests/helpers.py::TIGHT_K), calibrated from both sides on every row's model, chunks and cache: the float32
    numpy oracle and ATen float32 (oracle/torch_ref.py, where it has the model's head) PASS it against the float64 oracle; the
    fp16-operand emulation (one fp16 product: precision F16) and the emulation that rounds only the weights of the input Linear and
    the matrix convolutions to fp16 (an F16X3 product with its lo(w) * x term dropped) FAIL it."""
    import torch
    from oracle import folded_oracle, kws_oracle, torch_ref
    from tests.helpers import oracle64
    from wekws_amd import pack
    cfg, sd, x, c0 = _calibration_case(row)
    chunks = row["chunks"]
    ry, rc = oracle64(cfg, sd, x, c0, chunks)
    y32, c32 = kws_oracle.forward_streaming(cfg, sd, x, chunks, c0)
    e32 = max(tight_errors(cfg, y32, c32, ry, rc))
    assert e32 <= TIGHT_K / 4, e32                        # (the float32 oracle, with a margin of 4)
    if "classifier" not in cfg:
        tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
        ys, c, t = [], None if c0 is None else torch.from_numpy(c0), 0
        with torch.no_grad():
            for n in chunks:
                y, c = torch_ref.forward(cfg, tsd, torch.from_numpy(x[:, t:t + n].copy()), c)
                ys.append(y)
                t += n
        et = max(tight_errors(cfg, torch.cat(ys, 1).numpy(), c.numpy(), ry, rc))
        assert et <= TIGHT_K / 4, et
    desc, blob = pack.pack(cfg, sd)
    for rounds in ("both", "weights"):
        ys, c, t = [], c0, 0
        for n in chunks:
            y, c = folded_oracle.forward(desc, blob, x[:, t:t + n], mm_dtype=np.float16, rounds=rounds, in_cache=c, with_cache=True)
            ys.append(y)
            t += n
        e16 = max(tight_errors(cfg, np.concatenate(ys, 1), c, ry, rc))
        assert e16 > 4 * TIGHT_K, (rounds, e16)


# ---------------------------------------------------------------------------------------------------------------------------------
# GRU and FSMN (route.h: gru_shape_plan / select_gru_route / gru_reserve_bytes, fsmn_shape_plan / select_fsmn_route), through
# wekws_hip_debug_gru_route / wekws_hip_debug_fsmn_route.  GRU records: family, nn, spw, tchunk (0: one launch), nchunks, slots,
# tiles, grid, pk | k2 << 1 | nf_in_kernel << 2.  FSMN records: tile frames, nt, utterances per workgroup, head slices, grid, LDS,
# tiles of the call.
GRU_EXPECT = {
    (1, 10): ["gru_pipe", 0, 1, 0, 0, 1, 1, 33, 7],         # streaming chunk: time-packed, the non-finite pass in the kernel
    (1, 98): ["gru_pipe", 0, 16, 0, 0, 1, 1, 33, 6],
    (256, 10): ["gru_pipe", 0, 4, 0, 0, 64, 64, 256, 3],     # 64 slots x 4 stages fill the device: the separate non-finite launch
    (256, 98): ["gru_pipe", 0, 16, 0, 0, 16, 16, 80, 6],
    (1024, 98): ["gru_pipe", 0, 16, 0, 0, 64, 64, 256, 2],
    (16384, 98): ["gru_f16", 2, 32, 0, 1, 0, 512, 512, 0],   # 8 rounds of slots or more: the layer-major kernels, two tiles each
}
FSMN_EXPECT = {
    (1, 10): [64, 1, 1, 8, 1, 45056, 1, 0, 0],              # one utterance: the CTC head over 8 workgroups
    (256, 10): [64, 1, 1, 1, 256, 45056, 1, 0, 0],
    (1024, 32): [64, 2, 2, 1, 512, 153600, 1, 0, 0],         # two utterances per workgroup
    (1024, 64): [64, 4, 1, 1, 1024, 149504, 1, 0, 0],
    (4096, 32): [64, 2, 2, 1, 2048, 153600, 1, 0, 0],
}


@pytest.mark.parametrize("name,B,T", rm.GRU_CALLS)
def test_gru_recipes_take_the_route_they_were_built_for(hooks, name, B, T):
    r = rm.gru_route(hooks, M[name], B, T)
    assert r["plan"] == "as_is" and rm.gru_record(r) == GRU_EXPECT[(B, T)], r
    assert r["eff"] == "f16x3"
    assert rm.gru_route(hooks, M[name], B, T, precision="f32")["family"] == "gru_f32"
    assert rm.gru_route(hooks, M[name], B, T, opts={"gru_pipe": 0})["family"] == "gru_f16"


@pytest.mark.parametrize("name,B,T", rm.FSMN_CALLS)
def test_fsmn_recipes_take_the_route_they_were_built_for(hooks, name, B, T):
    r = rm.fsmn_route(hooks, M[name], B, T)
    assert r["plan"] == "as_is" and rm.fsmn_record(r) == FSMN_EXPECT[(B, T)] and r["ws"] == 0 and r["eff"] == "f16x3", r
    assert rm.fsmn_route(hooks, M[name], B, T, precision="f32")["plan"] == "generic"


def _gru_cfg(layers=2, hidden=128):
    cfg = copy.deepcopy(M["gru_2x128"])
    cfg["backbone"]["num_layers"] = layers
    cfg["hidden_dim"] = hidden
    return cfg


def test_gru_shape_plan(hooks):
    assert rm.gru_route(hooks, _gru_cfg(hidden=64), 3, 20)["plan"] == "padded"
    for cfg in (_gru_cfg(layers=5), _gru_cfg(hidden=160)):
        r = rm.gru_route(hooks, cfg, 3, 20)
        assert r["plan"] == "generic" and r["why"], r


@pytest.mark.parametrize("layers,hidden", [(1, 128), (2, 128), (2, 64), (4, 128)])
def test_gru_reservation_covers_every_smaller_call(hooks, layers, hidden):
    """wekws_hip_reserve(B, T) must hold every call of b <= B streams and t <= T frames, although a call's scratch is not
    monotonic in (B, T) (gru_f16_spw, the wavefront's slots): every (B, T) of the grid against the maxima over all smaller calls."""
    cfg = _gru_cfg(layers, hidden)
    Bmax, Tmax = 4200, 40
    need = np.zeros((Bmax, Tmax, 2), np.int64)
    res = np.zeros((Bmax, Tmax, 2), np.int64)
    for B in range(1, Bmax + 1):
        for T in range(1, Tmax + 1):
            r = rm.gru_route(hooks, cfg, B, T, reserve=True)
            need[B - 1, T - 1] = r["plain"], r["gran"]
            res[B - 1, T - 1] = r["res_plain"], r["res_gran"]
    cover = np.maximum.accumulate(np.maximum.accumulate(need, axis=0), axis=1)
    short = np.argwhere(res < cover)
    assert short.size == 0, [(int(b) + 1, int(t) + 1, "plain gran".split()[k]) for b, t, k in short[:10]]
    assert (need[:, :16] != cover[:, :16]).any()                  # (the non-monotonic case is in the grid)


def test_gru_wavefront_invariants(hooks):
    """The wavefront runs only where gru_pipe_geom admits it; its non-finite pass runs inside the launch only where every tile has a
    slot of its own (tiles <= slots) and the extra workgroups find CUs beside the stages.  At the MI355X partition sizes (32 .. 256
    CUs) the tiles <= slots bound never decides -- the CU bound alone gives the same answer for every B up to 70,000 --; at 384 CUs
    it does."""
    decides = {}
    for layers in (1, 2, 3, 4):
        cfg = _gru_cfg(layers)
        for cus in (32, 64, 128, 256, 384):
            for T in (10, 98):
                n = 0
                for B in range(1, 70001):
                    r = rm.gru_route(hooks, cfg, B, T, cus=cus)
                    if r["family"] != "gru_pipe":
                        assert r["family"] == "gru_f16" and not r["nf_in_kernel"] and B > 8 * min(cus // (2 * layers), 128), (B, cus)
                        continue
                    smax = min(cus // r["stages"], 128)
                    assert r["stages"] == 2 * layers and 1 <= r["slots"] <= smax and r["slots"] == min(r["tiles"], smax)
                    assert r["tiles"] <= 8 * r["slots"] and r["slots_p"] % 8 == 0 and r["slots_p"] >= r["slots"]
                    fits = (r["stages"] + 1) * r["slots"] <= cus
                    if r["nf_in_kernel"]:
                        assert r["tiles"] <= r["slots"] and fits
                    n += fits and not r["nf_in_kernel"]
                    assert r["grid"] == r["stages"] * r["slots_p"] + (r["slots"] if r["nf_in_kernel"] else 0)
                decides[(layers, cus, T)] = n
    assert all(n == 0 for (_, cus, _), n in decides.items() if cus <= 256), decides
    assert any(n for (_, cus, _), n in decides.items() if cus == 384), decides


def test_fsmn_route_invariants(hooks):
    """Over the FSMN recipes and longer memories: LDS within kFsmnLdsLimit, nt u <= 4, tiles chained through the workspace exactly
    when a call is longer than one tile; memories beyond the kernel's taps take the any-shape path."""
    cfgs = [M[n] for n in M if M[n]["backbone"]["type"] == "fsmn"]
    assert len(cfgs) >= 3
    for base in list(cfgs):
        for lo in (20, 40):
            cfg = copy.deepcopy(base)
            cfg["backbone"]["left_order"] = lo
            cfgs.append(cfg)
    generic = 0
    for cfg in cfgs:
        for B in (1, 2, 255, 256, 513, 1024, 4096):
            for T in (1, 16, 17, 32, 33, 64, 65, 130):
                r = rm.fsmn_route(hooks, cfg, B, T)
                if r["plan"] == "generic":
                    assert r["why"]
                    generic += 1
                    continue
                assert 1 <= r["max_nt"] <= 4 and r["tile_frames"] == 16 * r["max_nt"] and r["ntiles"] == -(-T // r["tile_frames"])
                assert r["u"] in (1, 2, 4) and r["nt"] * r["u"] <= 4 and r["nt"] * r["u"] <= r["max_nt"] or r["u"] == 1
                assert 0 < r["lds"] <= 160 * 1024 - 2048 and r["grid"] == -(-B // r["u"]) and r["head_slices"] >= 1
                assert (r["ws"] > 0) == (r["ntiles"] > 1)
                last = rm.fsmn_route(hooks, cfg, B, T, tile=r["ntiles"] - 1)
                assert 16 * last["nt"] >= T - (r["ntiles"] - 1) * r["tile_frames"] and 0 < last["lds"] <= 160 * 1024 - 2048
    assert generic


@pytest.mark.parametrize("seed", range(10))
def test_effective_precision_agrees_with_the_routes(hooks, seed):
    """F16 exactly when some call of the model under its options takes a one-product route (split 0)."""
    rng = np.random.default_rng([0xEF, seed])
    for _ in range(60):
        cfg, _ = random_model_config(rng)
        if cfg["backbone"]["type"] in ("gru", "fsmn"):
            continue
        opts = [int(rng.integers(0, 2)), 1, 1, 0, int(rng.integers(0, 2)), int(rng.integers(0, 2)), -1, 0, 0]
        r0 = route(hooks, cfg, 1, 1, precision="f16", opts=opts)
        if r0["plan"] == "generic":
            continue
        split0 = False
        for B in (1, 3, 257):
            for T in (1, 16, 17, 33, 65, 112):
                for hi, ho, x16, c16, nti in ((0, 1, 1, 1, 1), (1, 1, 1, 1, 1), (0, 1, 0, 1, 1), (1, 1, 0, 0, 1), (1, 1, 1, 1, 2), (0, 0, 1, 1, 1)):
                    r = route(hooks, cfg, B, T, has_in=hi, has_out=ho, precision="f16", x16=x16, cache16=c16, ntiles=nti, opts=opts)
                    split0 |= r["family"] != "none" and r["split"] == 0
        assert r0["eff"] == ("f16" if split0 else "f16x3"), (cfg, opts)
        assert route(hooks, cfg, 1, 1, precision="f32")["eff"] == "f32"
        assert route(hooks, cfg, 1, 1, precision="default")["eff"] == "f16x3"


# ---------------------------------------------------------------------------------------------------------------------------------
# the GRU / FSMN route matrix (tests/route_matrix_rnn.py)
from tests import route_matrix_rnn as rr  # noqa: E402

RNN_IDS = [r["id"] for r in rr.ROWS]


@pytest.mark.parametrize("row", rr.ROWS, ids=RNN_IDS)
def test_gru_fsmn_matrix_predictions_are_route_h(hooks, row):
    """The literal record of every chunk (FSMN: of every tile) is what route.h chooses for the call the forward makes."""
    assert rr.predict(hooks, row) == rr.EXPECT[row["id"]]


def _gru_reachable(lib):
    """Every (family, nn, spw, chunked, nchunks > 1, pk, k2, nf_in_kernel, tiles > slots) select_gru_route reaches over 1 .. 4
    layers, the stream counts at the edges of its choices, short and long inputs, both precisions, the three values of option
    gru_pipe, aligned and unaligned features and the four feature widths."""
    import itertools
    seen = {}
    for layers in (1, 2, 3, 4):
        smax = min(rm.CUS // (2 * layers), 128)                   # gru_pipe_geom: the wavefront's resident slots
        Bs = {1, 2, 3, 15, 16, 17, 4096, 4097, 16383, 16384}
        for k in (1, 2, 4, 8, 16, 8 * 16):                        # slots x streams per tile; 8 rounds of full tiles
            Bs |= {smax * k - 1, smax * k, smax * k + 1}
        for k in (1, 2, 4, 8, 16):                                # gru_f16_spw: 128 packed workgroups
            Bs |= {128 * k - 1, 128 * k, 128 * k + 1}
        for idim in (40, 64, 80, 23):
            cfg = _gru_cfg(layers)
            cfg["input_dim"] = idim
            for B, T, p, gp, x16 in itertools.product(sorted(Bs), (1, 8, 16, 17, 31, 32, 98), ("default", "f32"), (0, 1, 2), (0, 1)):
                r = rm.gru_route(lib, cfg, B, T, precision=p, x16=x16, opts={"gru_pipe": gp})
                assert r["plan"] == "as_is" and r["family"] != "none", r
                seen.setdefault(rr.gru_tuple(rm.gru_record(r)), (layers, idim, B, T, p, gp, x16))
    return seen


def _fsmn_reachable(lib):
    """Every (max_nt, nt, u, head_slices > 1, tile index > 0, ntiles > 1) select_fsmn_route reaches over the configurations and the
    B / T grid of test_fsmn_route_invariants."""
    cfgs = [M[n] for n in M if M[n]["backbone"]["type"] == "fsmn"]
    for base in list(cfgs):
        for lo in (20, 40):
            cfg = copy.deepcopy(base)
            cfg["backbone"]["left_order"] = lo
            cfgs.append(cfg)
    seen = {}
    for cfg in cfgs:
        for B in (1, 2, 255, 256, 513, 1024, 4096):
            for T in (1, 16, 17, 32, 33, 64, 65, 130):
                first = rm.fsmn_route(lib, cfg, B, T)
                if first["plan"] == "generic":
                    continue
                for i in range(first["ntiles"]):
                    r = rm.fsmn_route(lib, cfg, B, T, tile=i)
                    seen.setdefault(rr.fsmn_tuple(rm.fsmn_record(r), i), (cfg["output_dim"], cfg["backbone"]["left_order"], B, T, i))
    return seen


def test_gru_fsmn_matrix_covers_every_reachable_route(hooks):
    """A route.h change that adds a GRU or FSMN variant fails here until a row runs it on the GPU -- and every route tuple has a row
    that compares per-frame logits (activation identity) of a head of at least 12 classes, and a control row."""
    for kind, reach, least in (("gru", _gru_reachable(hooks), 31), ("fsmn", _fsmn_reachable(hooks), 19)):
        rows = [r for r in rr.ROWS if r["kind"] == kind]
        have = set().union(*(rr.row_tuples(r) for r in rows))
        missing = {t: reach[t] for t in reach if t not in have}
        assert not missing, missing
        assert len(reach) >= least, (kind, len(reach))                  # (the sweep cannot shrink silently)
        logits = set().union(*(rr.row_tuples(r) for r in rows if rr.is_identity(r) and rr.row_config(r)["output_dim"] >= 12))
        assert have == logits, have - logits
        control = set().union(*(rr.row_tuples(r) for r in rr.control_rows() if r["kind"] == kind))
        assert have == control, have - control
        assert {rr.EXPECT[r["id"]][0] for r in rows} == ({"as_is", "padded", "generic"} if kind == "gru" else {"as_is", "generic"})


def test_gru_fsmn_matrix_rows_cover_the_edges():
    G, F = rr.GRU_ROWS, rr.FSMN_ROWS
    rec = [(r, dict(zip(rm.GRU_REC, c))) for r in G for c in rr.EXPECT[r["id"]][1] if c]
    fam = lambda f: [(r, d) for r, d in rec if d["family"] == f]                      # noqa: E731
    assert {d["nn"] for _, d in fam("gru_f32")} == {1, 4} and {d["nn"] for _, d in fam("gru_f16")} == {1, 2}
    assert {d["spw"] for r, d in fam("gru_f16") if max(r["chunks"]) <= 16 and d["nn"] == 1} == {1, 2, 4, 8, 16}
    assert any(d["tchunk"] and sum(r["chunks"]) % d["tchunk"] for r, d in fam("gru_f16"))          # the last time chunk is shorter
    assert any(not d["tchunk"] and max(r["chunks"]) >= 32 for r, d in fam("gru_f16"))
    assert {d["spw"] for _, d in fam("gru_pipe")} == {1, 2, 4, 8, 16}
    assert {(d["bits"] & 1, d["bits"] >> 1 & 1, d["bits"] >> 2 & 1) for _, d in fam("gru_pipe")} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    assert any(d["tiles"] > 8 * d["slots"] and r["opts"].get("gru_pipe") == 2 for r, d in fam("gru_pipe"))
    assert any(d["slots"] < d["tiles"] <= 8 * d["slots"] for _, d in fam("gru_pipe"))
    k2_0 = {(rr.row_config(r)["input_dim"], r["x_off"]) for r, d in fam("gru_pipe") if not d["bits"] >> 1 & 1}
    assert {(80, 0), (23, 0), (40, 1)} <= k2_0
    assert {40, 64} <= {rr.row_config(r)["input_dim"] for r, d in fam("gru_pipe") if d["bits"] >> 1 & 1}
    assert {rr.row_config(r)["backbone"]["num_layers"] for r in G} == {1, 2, 3, 4, 5}
    assert {rr.row_config(r)["hidden_dim"] for r in G} == {64, 128, 160}
    assert any(rr.EXPECT[r["id"]][0] == "padded" and r["state"] for r in G)
    odims = {rr.row_config(r)["output_dim"] for r in G}
    assert {1, 2, 17} <= odims and max(odims) > 128
    assert {1, 2, 3, 15, 16, 17, 33} <= {t for r in G for t in r["chunks"]} and any(t > 2 * 16 + 16 for r in G for t in r["chunks"])
    assert any(r["B"] == 1 for r in G) and any(r["B"] % 16 for r in G) and any(d["slots"] and r["B"] % d["slots"] == 1 for r, d in rec)
    assert any(r["chunks"] == [10, 10, 10] for r in G) and {0.5, 3.0, None} == {r["state"] for r in G}
    frec = [(r, dict(zip(rm.FSMN_REC, t)), i) for r in F for ch in rr.EXPECT[r["id"]][1] for i, t in enumerate(ch)]
    assert {d["nt"] for _, d, _ in frec} == {1, 2, 3, 4} and {d["u"] for _, d, _ in frec} == {1, 2, 4}
    assert any(d["u"] > 1 and sum(r["chunks"][:1]) % 16 for r, d, _ in frec)
    assert {1, 3, 8} <= {d["head_slices"] for _, d, _ in frec} and any("head_slices" in r["opts"] for r in F)
    assert {2, 3} <= {d["ntiles"] for _, d, _ in frec} and any(i and i == d["ntiles"] - 1 and 16 * d["nt"] < d["tile_frames"] for _, d, i in frec)
    assert {2, 3, 4} <= {d["tile_frames"] // 16 for _, d, _ in frec}
    assert any(r["state"] for r in F) and any(r["state"] is None for r in F) and any(len(r["chunks"]) > 1 for r in F)
    assert any(r["x_off"] for r in F) and any(r["c_off"] and r["state"] for r in F)
    assert any(rr.row_config(r)["backbone"]["linear_dim"] % 32 for r in F)                      # padded widths
    generic = [r for r in F if rr.EXPECT[r["id"]][0] == "generic"]
    assert any(r["precision"] == "f32" for r in generic) and any(rr.row_config(r)["backbone"]["left_order"] > 32 for r in generic)


@pytest.mark.parametrize("row", rr.ROWS, ids=RNN_IDS)
def test_tight_bar_holds_f32_and_rejects_one_rounded_matrix(row):
    """TIGHT_K on every GRU / FSMN row (at most 4 utterances: the bar is per element), from both sides.  (a) The float32 numpy
    oracle, and ATen float32 where oracle/torch_ref.py has the model, are within TIGHT_K / 4 of the float64 oracle.  (b) The
    float32 oracle with ONE weight matrix rounded to fp16 -- an F16X3 product that dropped its lo(w) * x term in one place: every
    matrix the kernels multiply on the matrix cores, one at a time -- misses the bar by a factor of at least 2, in the outputs or in
    the returned state.  (The factor is 2 and not the conv calibration's 4: one matrix is a much smaller defect than the
    whole-network emulations used there.  The classifier of a sigmoid row is left out: rr.defect_visibility.)"""
    cfg, sd, x, s0 = rr.calibration_case(row)
    rys, rcs = rr.reference(cfg, sd, x, s0, row["chunks"], np.float64)
    ys, cs = rr.reference(cfg, sd, x, s0, row["chunks"], np.float32)
    e32 = rr.row_error(row, cfg, ys, cs, rys, rcs)
    assert e32 <= TIGHT_K / 4, e32
    aten = rr.aten_reference(cfg, sd, x, s0, row["chunks"])
    assert (aten is not None) == (row["kind"] == "gru")
    if aten is not None:
        et = rr.row_error(row, cfg, aten[0], aten[1], rys, rcs)
        assert et <= TIGHT_K / 4, et
    vis = rr.defect_visibility(row, (cfg, sd, x, s0), (rys, rcs))
    assert len(vis) == len(rr.matrices(cfg, sd)) - (row["kind"] == "gru" and not rr.is_identity(row))
    weak = {k: v / TIGHT_K for k, v in vis.items() if v < 2 * TIGHT_K}
    assert not weak, weak
