"""CPU: the poisoned matrix (tests/nonfinite_matrix.py) -- that it reaches every kernel route with a non-finite input, that its
placements rotate as its docstring says, and that the comparison the GPU test makes (tests/test_hip_nonfinite_matrix.py:
classes, then the masked tight bar, tests/helpers.py::masked_tight_error) is calibrated from three sides:
  * reference side: on every derived row and every golden case the float32 oracle has the float64 oracle's classes and stays
    under TIGHT_K / 2, and every "reached through the cache alone" claim of a row is true of the float64 oracle;
  * defect side: CPU emulations of what the device code exists to prevent show as class mismatches;
  * value side: one weight matrix rounded to fp16 misses the bar on the finite values of the poisoned utterances alone."""
import copy

import numpy as np
import pytest

from oracle import kws_oracle
from tests import nonfinite_matrix as nm
from tests import route_matrix as rm
from tests import route_matrix_rnn as rr
from tests.golden.nonfinite_cases import CASES, poisoned_input
from tests.helpers import CONTROL_MARGIN, TIGHT_K, cache_axis, case_weights, golden_oracle64, masked_tight_error, value_classes, y_axis

ROW_IDS = [r["id"] for r in nm.ROWS]


@pytest.fixture(scope="module")
def hooks():
    return nm.hooks()


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage
def test_every_route_tuple_meets_poison(hooks, capsys):
    """Every route tuple of the two matrices: some derived row puts a poisoned utterance into a segment of that route through
    the features, and -- where a segment of that route has an incoming cache or state -- some row through that alone.  The
    routes are the matrices' own tuples; the table counts them by the coarser keys nm.issue_key.  A route.h change that adds a
    variant fails tests/test_route.py until a finite row exists and fails HERE until its poisoned row does (the sweeps of
    test_route.py are repeated against the poisoned rows)."""
    from tests import test_route as tr
    need, got = nm.universe(), nm.reached()
    assert not need - got, sorted(need - got, key=repr)
    sweeps = {"conv": tr._reachable(hooks), "gru": tr._gru_reachable(hooks), "fsmn": tr._fsmn_reachable(hooks)}
    f16_only = set()
    for row in rm.ROWS:
        if rm.is_split_row(row):
            f16_only.update(rm.route_tuple(t) for ch in rm.predict(hooks, row, "f16")[1] for t in ch)
    f16_only -= {t for k, v, t in need if k == "conv"}
    table = {}
    for kind, reach in sweeps.items():
        missing = {t: reach[t] for t in reach if (kind, "x", t) not in got and t not in f16_only}
        assert len(reach) >= (140, 31, 19)[("conv", "gru", "fsmn").index(kind)]
        assert not missing, (kind, missing)
        route = lambda t: t != nm.ANY and t[0] != "padded"                               # noqa: E731
        keys = {nm.issue_key(kind, t) for k, v, t in need if k == kind and route(t)}
        have = {nm.issue_key(kind, t) for k, v, t in got if k == kind and v == "x" and route(t)}
        table[kind] = (len(keys & have), len(keys))
    with capsys.disabled():
        print("\nroute tuples reached by a non-finite row: " + ", ".join(f"{k} {a}/{b}" for k, (a, b) in table.items()))
    assert all(a == b for a, b in table.values()), table
    assert table["conv"][1] >= 92 and table["gru"][1] >= 31 and table["fsmn"][1] >= 18, table      # (the matrices cannot shrink silently)
    assert {("conv", "x", nm.ANY), ("gru", "x", nm.ANY), ("fsmn", "x", nm.ANY)} <= got
    f16 = [r for r in nm.ROWS if r["precision"] == "f16"]
    fams = {t.split()[0] for r in f16 for ch in nm.expect(r, hooks)[1] for t in ch if t.endswith("split0")}
    assert fams == set(rm.ONE_PRODUCT), fams


def test_cheapest_row_per_tuple():
    """Every plan of every derived row is there for something that no plan of any row reaches at a lower nm.plan_rank (B = 1
    streams kept clean, identity heads, then B x frames): nothing is run that a cheaper row would have served."""
    order = lambda base, mode, s: nm.plan_rank(base, mode, s)[:3]                     # noqa: E731  (without the tie-break by name)
    best = {}
    for base in rm.ROWS + rr.ROWS:
        for mode, s, got in nm._candidates(base):
            for need in got:
                best[need] = min(best.get(need, (2, 0, 0)), order(base, mode, s))
    for row in nm.ROWS:
        if row["precision"] != row["base"]["precision"]:
            continue
        for mode, s in row["plans"]:
            reach = [got for m2, s2, got in nm._candidates(row["base"]) if (m2, s2) == (mode, s)][0]
            assert any(order(row["base"], mode, s) == best[need] for need in reach), (row["id"], mode, s)


def test_placements_rotate():
    rows = nm.ROWS
    xs = [p for r in rows for p in r["poison"] if p[0] == "x"]
    cs = [(r, p) for r in rows for p in r["poison"] if p[0] == "c"]
    assert {p[4] for p in xs} == set(range(5)) and {p[2] for _, p in cs} == set(range(5))
    assert [int(np.isnan(v)) for v in nm.VALUES] == [1, 1, 1, 0, 0] and np.signbit(nm.VALUES[1]) and nm.VALUES.view(np.uint32)[2] == 0x7f800001
    for r in rows:
        B, bad, base = r["base"]["B"], r["bad"], r["base"]
        segs = nm.segments(base)
        assert bad == sorted(set(bad)) and all(0 <= u < B for u in bad)
        if B >= 3:
            assert {0, B - 1} <= set(bad) and any(u not in bad for u in range(1, B - 1)), r["id"]       # a clean neighbour in between
        if nm._persistent(base):
            walk = list(range(0, B, rm.CUS))
            assert {walk[0], walk[len(walk) // 2], walk[-1], B - 1} == set(bad)
        if r["kind"] == "gru" and B > 16:
            assert {0, 15, 16} <= set(bad)
        xseg = [(segs[q][1], segs[q][2]) for m, q in r["plans"] if m == "x"]
        for p in r["poison"]:
            assert (p[1] if p[0] == "x" else p[1][1] if r["kind"] == "gru" else p[1][0]) in bad
            if p[0] == "x":
                assert any(a <= p[2] < b for a, b in xseg)
        # B = 1: the earlier chunks stay a clean stream, unless something the row reaches is reached by no plan that keeps them so
        for mode, q in r["plans"]:
            if B == 1 and segs[q][0] != len(base["chunks"]) - 1 and r["precision"] == base["precision"]:      # (f16 reruns: nm.derive)
                mine = [got for m2, s2, got in nm._candidates(base) if (m2, s2) == (mode, q)][0]
                for b2 in rm.ROWS + rr.ROWS:
                    for m2, s2, got in nm._candidates(b2):
                        if not (b2["B"] == 1 and nm.segments(b2)[s2][0] != len(b2["chunks"]) - 1):
                            mine = mine - got
                assert mine, r["id"]
    # first / last / middle elements, in the features and in the states
    places = set()
    for r in rows:
        ends = {(nm.segments(r["base"])[q][1], nm.segments(r["base"])[q][2]) for m, q in r["plans"] if m == "x"}
        for p in r["poison"]:
            if p[0] == "x":
                places.add("first" if p[3] == 0 and any(p[2] == a for a, _ in ends) else
                           "last" if p[3] > 0 and any(p[2] == b - 1 for _, b in ends) else "middle")
    assert places == {"first", "last", "middle"}
    # multi-utterance workgroups: B no multiple of the utterances per workgroup, the poison in the last utterance
    assert any(nm._upw(r["base"]) > 1 and r["base"]["B"] % nm._upw(r["base"]) and r["base"]["B"] - 1 in r["bad"] and r["base"]["B"] > 1
               for r in rows if r["kind"] == "conv")
    # persistent rows of both families with NfList code
    pers = {nm.segments(r["base"])[q][3][0] for r in rows if nm._persistent(r["base"]) for _, q in r["plans"]}
    assert {"ds256_g16", "ds256_g32"} <= pers
    # GRU: the last stream of a partial tile; h0 in the first and in the last layer; a frame of a later time chunk
    g = [r for r in rows if r["kind"] == "gru"]
    assert any(r["base"]["B"] % 16 and r["base"]["B"] > 16 for r in g)
    layers = {(p[1][0] == 0, p[1][0] == nm.state_shape(r["base"], rr.row_config(r["base"]))[0] - 1) for r, p in cs if r["kind"] == "gru"}
    assert {(True, False), (False, True)} <= layers or (True, True) in layers and len(layers) > 1
    chunked = [(r, nm.segments(r["base"])[q]) for r in g for m, q in r["plans"] if m == "x"]
    chunked = [(r, s) for r, s in chunked if s[5] is not None and s[5][3] and s[2] - s[1] > s[5][3]]
    assert chunked and all(p[2] - s[1] >= s[5][3] for r, s in chunked for p in r["poison"] if p[0] == "x")


# ---------------------------------------------------------------------------------------------------------------------------------
# calibration, reference side
def _subcase(row):
    """The row at calibration_subset's utterances: (cfg, sd, x, c0, poisoned utterances as indices INTO the subset)."""
    cfg, sd, x, c0, _, _ = nm.row_case(row)
    pick = nm.calibration_subset(row)
    bad = [pick.index(u) for u in row["bad"] if u in pick]
    return cfg, sd, x[pick], nm.take(row["kind"], c0, pick), bad


def row_errors(row, cfg, ys, cs, rys, rcs, bad=None):
    """The largest masked tight error over every chunk's output and the state after every chunk (bad: over those utterances
    alone); inf on a class mismatch.  The four CTC-head stream rows of the FSMN matrix take each class's scale over the stream."""
    kind = row["kind"]
    scale = np.concatenate(rys, axis=1) if row["base"].get("stream_scale") else None
    worst = 0.0
    for y, ry, c, rc in zip(ys, rys, cs, rcs):
        wy = None if bad is None else nm.utt_mask(kind, ry.shape, bad)
        wc = None if bad is None else nm.utt_mask(kind, rc.shape, bad, state=True)
        worst = max(worst, masked_tight_error(y, ry, y_axis(cfg), wy, scale), masked_tight_error(c, rc, cache_axis(cfg), wc))
    return worst


REFS = {}


def refs64(row):
    if row["id"] not in REFS:
        cfg, sd, x, c0, bad = _subcase(row)
        REFS[row["id"]] = (cfg, sd, x, c0, bad, nm.reference(cfg, sd, x, c0, row["base"]["chunks"], np.float64))
    return REFS[row["id"]]


@pytest.mark.parametrize("row", nm.ROWS, ids=ROW_IDS)
def test_reference_side(row):
    """The float32 oracle against the float64 oracle on the poisoned row (at most 4 utterances): the same classes everywhere and
    under TIGHT_K / 2 -- the yardstick itself does not depend on its arithmetic type where non-finite values travel.  And the row's
    claims hold: a segment it claims through the features has the poison in its features, one it claims through the cache has
    clean features and a non-finite incoming cache / state in the float64 oracle."""
    cfg, sd, x, c0, bad, (rys, rcs) = refs64(row)
    ys, cs = nm.reference(cfg, sd, x, c0, row["base"]["chunks"], np.float32)
    e32 = row_errors(row, cfg, ys, cs, rys, rcs)
    assert e32 <= TIGHT_K / 2, e32
    segs = nm.segments(row["base"])
    _, states = nm.reference(cfg, sd, x, c0, nm.segment_chunks(row), np.float64)
    incoming = [c0] + states[:-1]
    pick = nm.calibration_subset(row)
    for s, via, utts in row["claims"]:
        a, b = segs[s][1:3]
        mine = [pick.index(u) for u in utts if u in pick]
        assert mine, (row["id"], s, utts, pick)
        xbad = [not np.isfinite(x[u, a:b]).all() for u in mine]
        cbad = [incoming[s] is not None and not np.isfinite(nm.take(row["kind"], incoming[s], [u])).all() for u in mine]
        if via == "x":
            assert any(xbad), (row["id"], s)
        else:
            assert any(c and not f for f, c in zip(xbad, cbad)), (row["id"], s, xbad, cbad)
    clean = [u for u in range(x.shape[0]) if u not in bad]
    for y in rys:
        assert np.isfinite(y[clean]).all()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_side_on_the_goldens(case):
    from tests.test_nonfinite_oracle import run_oracle
    cfg, sd = case_weights(case)
    x, c0 = poisoned_input(case, cfg)
    y32, c32 = run_oracle(case, cfg, sd, x, c0)
    y64, c64 = golden_oracle64(case, cfg, sd, x, c0)
    e = max(masked_tight_error(y32, y64, y_axis(cfg, case.get("softmax", False))), masked_tight_error(c32, c64, cache_axis(cfg)))
    assert e <= TIGHT_K / 2, e



# ---------------------------------------------------------------------------------------------------------------------------------
# calibration, value side
def matrices(cfg, sd):
    """The weight matrices of a model (everything the kernels multiply on the matrix cores; depthwise taps and the FSMN memory
    taps are vector arithmetic)."""
    if cfg["backbone"]["type"] in ("gru", "fsmn"):
        return rr.matrices(cfg, sd)
    return [k for k, v in sd.items() if k.endswith("weight") and np.ndim(v) >= 2 and np.shape(v)[1] > 1]


def value_visibility(row, stop_at=None):
    """{matrix: error of the float32 oracle with that one matrix rounded to fp16, on the FINITE values of the poisoned utterances
    alone, against the float64 oracle of the unrounded weights} (stop_at: stop at the first matrix that reaches it); and the
    number of finite reference values those utterances have."""
    cfg, sd, x, c0, bad, (rys, rcs) = refs64(row)
    kind = row["kind"]
    finite = sum(int(np.isfinite(y[bad]).sum()) for y in rys) + sum(int(np.isfinite(nm.take(kind, c, bad)).sum()) for c in rcs)
    out = {}
    names = matrices(cfg, sd)
    for name in names[::-1]:                     # (the head first: the matrix every finite output has gone through)
        ys, cs = nm.reference(cfg, rr.rounded(sd, name), x, c0, row["base"]["chunks"], np.float32)
        out[name] = row_errors(row, cfg, ys, cs, rys, rcs, bad)
        if stop_at is not None and out[name] >= stop_at:
            break
    return out, finite


@pytest.mark.parametrize("row", nm.ROWS, ids=ROW_IDS)
def test_value_side(row):
    """Classes alone would pass a repair that returns wrong FINITE values next to the right NaNs.  On every row, on the finite
    values of the poisoned utterances alone, the float32 oracle with ONE weight matrix rounded to fp16 (a product that lost its
    lo(w) term) misses the tight bar by CONTROL_MARGIN for some matrix: what those utterances keep finite is enough to see a
    precision defect of the repair.  The exception is a rule, not a list: nm.nothing_to_see."""
    if nm.nothing_to_see(row):
        return
    vis, finite = value_visibility(row, CONTROL_MARGIN * TIGHT_K)
    assert finite and max(vis.values()) >= CONTROL_MARGIN * TIGHT_K, {k: v / TIGHT_K for k, v in vis.items()}


def test_value_side_exceptions_are_few():
    blind = [r["id"] for r in nm.ROWS if nm.nothing_to_see(r)]
    assert len(blind) <= 8, blind


# ---------------------------------------------------------------------------------------------------------------------------------
# calibration, defect side: CPU emulations of what the device code exists to prevent must show as CLASS mismatches
def _classes_differ(ys, cs, rys, rcs):
    return any(not np.array_equal(value_classes(a), value_classes(b)) for a, b in zip(ys + cs, rys + rcs) if a.shape == b.shape)


def _passes_a_relu(row):
    """The row has a NaN that meets a ReLU: in the features, or in a conv / FSMN cache (a GRU state meets none)."""
    return any(p[-1] <= 2 and (p[0] == "x" or row["kind"] != "gru") for p in row["poison"])


NAN_ROWS = [r for r in nm.ROWS if _passes_a_relu(r)]


@pytest.mark.parametrize("row", NAN_ROWS, ids=[r["id"] for r in NAN_ROWS])
def test_defect_fmax_relu_is_a_class_mismatch(row, monkeypatch):
    """A missed detection: the kernels' ReLU is v_max_f32, which returns the operand that is a number -- relu(NaN) = 0.  The
    oracle with that ReLU (np.fmax) returns finite values where the reference has NaN, on every row with a NaN that meets one."""
    cfg, sd, x, c0, bad, (rys, rcs) = refs64(row)
    monkeypatch.setattr(kws_oracle, "relu", lambda v, dt=np.float32: np.fmax(v, dt(0)))
    ys, cs = nm.reference(cfg, sd, x, c0, row["base"]["chunks"], np.float32)
    assert _classes_differ(ys, cs, rys, rcs)


def test_nan_rows_are_most_rows():
    """(The values cycle, so a row of one poisoned utterance may hold an Inf alone: +Inf passes a ReLU as it is, and -Inf leaves
    through one as 0 -- rows whose reference is finite everywhere exist, and the device must return that too.)"""
    assert len(NAN_ROWS) >= len(nm.ROWS) // 2
    assert {r["kind"] for r in NAN_ROWS} == {"conv", "gru", "fsmn"}


def padded_model(hooks, row):
    """The row's model as the kernels run a shape no kernel is built for: hidden width and kernel size of the next built shape
    (route.h's plan), every new weight exactly zero, the extra taps the OLDEST ones (a BatchNorm's new channels: variance 1)."""
    base = row["base"]
    cfg = rm.row_config(base)
    sd = rm.row_weights(base, cfg)
    r = rm.route(hooks, cfg, base["B"], 1, precision=row["precision"])
    assert r["plan"] == "padded"
    C, ks, Cp, ksp = cfg["hidden_dim"], cfg["backbone"]["kernel_size"], r["C"], r["ks"]
    wide = copy.deepcopy(cfg)
    wide["hidden_dim"] = Cp
    wide["backbone"]["kernel_size"] = ksp
    if "hidden_dim" in wide["backbone"]:
        wide["backbone"]["hidden_dim"] = Cp
    out = {}
    for k, v in sd.items():
        v = np.asarray(v)
        pads = [(0, Cp - n) if n == C and C != Cp else (0, 0) for n in v.shape]
        if v.ndim == 3 and v.shape[2] == ks and ksp != ks and "cnn.0" in k or (v.ndim == 3 and v.shape[2] == ks and ksp != ks and "conv1.conv" in k):
            pads[2] = (ksp - ks, 0)
        out[k] = np.pad(v, pads, constant_values=1.0 if k.endswith("running_var") else 0.0) if v.ndim else v
    return cfg, sd, wide, out


PADDED_ROWS = [r for r in nm.ROWS if r["kind"] == "conv" and nm.base_expect(r["base"])[0] == "padded"]


@pytest.mark.parametrize("row", PADDED_ROWS, ids=[r["id"] for r in PADDED_ROWS])
def test_defect_zero_padded_weights_are_a_class_mismatch(row, hooks):
    """skip_zero off: 0 x NaN.  The oracle on the zero-padded weights computes the SAME function on finite inputs (checked first).
    With poison it differs in class where the KERNEL SIZE is padded: the zero taps reach (8 - 5) x 15 frames further back than
    the model's, and frames the reference has finite again come back NaN (the row poisons an early frame of its first call for
    this).  Where only the WIDTH is padded the emulation cannot differ in what the caller sees, and the test says so: the first
    pointwise / dense convolution spreads a NaN over all channels in the caller's model too, and the new channels are cropped."""
    cfg, sd, wide, wsd = padded_model(hooks, row)
    _, _, x, c0, x0, _ = nm.row_case(row)
    assert c0 is None
    chunks = row["base"]["chunks"]
    ys0, _ = nm.reference(cfg, sd, x0, None, chunks, np.float64)
    yw0, _ = nm.reference(wide, wsd, x0, None, chunks, np.float64)
    assert max(float(np.abs(a - b).max()) for a, b in zip(ys0, yw0)) <= 1e-12                   # the same model
    rys, _ = nm.reference(cfg, sd, x, None, chunks, np.float64)
    yw, _ = nm.reference(wide, wsd, x, None, chunks, np.float64)
    differ = any(not np.array_equal(value_classes(a), value_classes(b)) for a, b in zip(yw, rys))
    assert differ == (wide["backbone"]["kernel_size"] != cfg["backbone"]["kernel_size"])


def test_a_padded_kernel_size_row_exists():
    assert any(rm.row_config(r["base"])["backbone"]["kernel_size"] not in (5, 8) or
               (rm.row_config(r["base"])["backbone"]["type"] == "tcn" and rm.row_config(r["base"])["backbone"]["kernel_size"] != 8)
               for r in PADDED_ROWS)


def test_defect_nosubsampling_through_the_matrix_is_a_class_mismatch():
    """NoSubsampling arrives at the kernels as a diagonal preprocessing matrix.  Through the full matrix product an Inf in one
    channel meets the zeros of every other row (0 x Inf = NaN in every channel of the frame); taken channel by channel it stays
    where it is.  On the golden case without a subsampling layer the two differ in class."""
    case = [c for c in CASES if c.get("no_subsampling")][0]
    cfg, sd = case_weights(case)
    x, c0 = poisoned_input(case, cfg)
    y, c = golden_oracle64(case, cfg, sd, x, c0)
    with np.errstate(all="ignore"):
        xm = np.matmul(x.astype(np.float64), np.eye(cfg["input_dim"])).astype(np.float32)
    ym, cm = golden_oracle64(case, cfg, sd, xm, c0)
    assert np.array_equal(value_classes(xm[0]), value_classes(x[0])) and not np.array_equal(value_classes(xm), value_classes(x))
    assert not np.array_equal(value_classes(cm), value_classes(c)) or not np.array_equal(value_classes(ym), value_classes(y))


# ---------------------------------------------------------------------------------------------------------------------------------
# the named stress rows (tests/tools/nonfinite_matrix_cases.py::STRESS) take the routes they are named for
def test_stress_rows_take_the_routes_they_are_named_for(hooks):
    from tests.tools.nonfinite_matrix_cases import NFLIST, STRESS, stress_predict
    for name, fam in (("nflist_g16", "ds256_g16"), ("nflist_g32", "ds256_g32")):
        kind, plan, chunks = stress_predict(hooks, name)
        B = STRESS[name][4]
        tiles = [rm.route_tuple(t) for ch in chunks for t in ch]
        assert kind == "conv" and all(t[0] == fam and t[5] == 1 for t in tiles), (name, chunks)      # the persistent variant
        assert all(" upw1 " in t for ch in chunks for t in ch) and B == 30 * rm.CUS + 1
        if name == "nflist_g16":
            assert [t[2] for t in tiles] == [0, 1]                                               # without and with the context
        # the walks of workgroups 0 / 1 / 2 (b = g, g + 256, ...): one more than the list holds, exactly the list, and a walk in
        # which noted and clean utterances alternate -- a clean one behind a noted one and a noted one behind a clean one
        walks = [[b in NFLIST for b in range(g, B, rm.CUS)] for g in range(3)]
        assert sum(walks[0]) == len(walks[0]) == 31 and sum(walks[1]) == len(walks[1]) == 30
        pairs = set(zip(walks[2], walks[2][1:]))
        assert {(True, False), (False, True)} <= pairs and sum(walks[2]) == 15
        assert all(not any(b in NFLIST for b in range(g, B, rm.CUS)) for g in range(3, rm.CUS))
    kind, _, chunks = stress_predict(hooks, "slots_conv_upw1")
    assert all(t.startswith("ds256") and " upw1 " in t and " pers0 " in t for ch in chunks for t in ch)
    kind, _, chunks = stress_predict(hooks, "slots_conv_upw2")
    assert kind == "conv" and all(" upw2 " in t and " pers0 " in t for ch in chunks for t in ch), chunks
    kind, _, chunks = stress_predict(hooks, "slots_gru_fix")
    recs = [dict(zip(rm.GRU_REC, c)) for c in chunks]
    assert kind == "gru" and all(d["family"] == "gru_f16" and not d["bits"] >> 2 & 1 for d in recs), chunks       # the separate fix launch
    kind, _, chunks = stress_predict(hooks, "slots_fsmn")
    assert kind == "fsmn" and all(dict(zip(rm.FSMN_REC, t))["u"] == 1 for ch in chunks for t in ch)
    # more poisoned workgroups than the 16 scratch slots, on every slots_* row
    for name in STRESS:
        if name.startswith("slots"):
            upw = 2 if name.endswith("upw2") else 1
            assert len({u // upw for u in STRESS[name][6]}) > 16 and STRESS[name][8] == 2 and len(STRESS[name][6]) == 40
