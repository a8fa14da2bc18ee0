"""The poisoned matrix: rows of the two route matrices (tests/route_matrix.py, tests/route_matrix_rnn.py) with NaN / +-Inf put into
their features or into their incoming cache / state, so that every kernel route meets a non-finite input (how the kernels deal
with one: wekws_amd/csrc/nonfinite.hip.h).  No row is written down here: ROWS is DERIVED from rm.ROWS and rr.ROWS.
A derived row keeps its base row's model, B, chunks, options, offsets, weights, inputs and predicted trace (poison must not change
the route) and adds a deterministic poison plan.

Segments.  A call is cut where the kernels cut it: a conv call into its 112-frame tiles, an FSMN call into its frame tiles, a GRU
call is one segment.  Every segment has the route tuple the base matrix predicts for it.  A poisoned utterance reaches a segment
  * "x": through the segment's own features (the plan puts the value there), or
  * "c": through the cache / state alone -- the incoming one of the call, or what an earlier segment handed over -- while the
    segment's own features are clean.
Coverage (tests/test_nonfinite_matrix.py): every route tuple of the matrices is reached through "x", and through "c" wherever a
segment of that route has an incoming cache or state at all; the cheapest base row (B x frames) is taken per tuple.  The claims
are checked against the float64 oracle there: the cache that enters a "c" segment really is non-finite.

Placement, rotating with a number taken from the derived row's name:
  * utterances: 0 and B - 1 with the clean ones in between (B = 2: one of the two; B = 1: the only one, and then the poison goes
    into the LAST chunk where the route allows it, so that the earlier chunks stay a clean stream); persistent conv rows (fewer
    workgroups than utterances): the first, a middle and the last utterance of workgroup 0's walk b = 0 mod 256, and B - 1 (at
    B = 257 and 513 that is the whole walk: a walk in which noted and clean utterances alternate is a stress row); GRU:
    streams 0, 15, 16 (the edge of a 16-stream tile) and B - 1 (the last stream of a partial tile);
  * elements: the first element of the segment, the last element of its last frame, a middle one -- one placement per poisoned
    utterance, rotating; where a later segment must receive the poison through the cache, the plan's first utterance takes
    the last frame (from the first frame of a 112-frame tile a DS-TCN cache is clean again: the receptive field is 106 frames);
    a time-chunked gru_f16 row takes frames of its later time chunks;
  * incoming state: GRU h0 alternately in the last and in the first layer; conv / FSMN caches at the first, last and a middle
    element of the utterance's block;
  * values, cycling: NaN, NaN with the sign bit set, the signalling NaN 0x7f800001, +Inf, -Inf.
GRU / FSMN rows whose base row has no incoming state take an all-zero one for the "c" plan (h0 = 0 / the empty cache are what
None means to those kernels, and their routes do not depend on it); conv rows are poisoned through the cache only where the base
row has one, since a conv route depends on it."""
import ctypes as C
import zlib

import numpy as np

from tests import route_matrix as rm
from tests import route_matrix_rnn as rr
from wekws_amd import pack

TILE = rm.TILE
BITS = (0x7fc00000, 0xffc00000, 0x7f800001, 0x7f800000, 0xff800000)      # NaN, -NaN, signalling NaN, +Inf, -Inf
VALUES = np.array(BITS, np.uint32).view(np.float32)
PLACES = ("first", "last", "middle")
ANY = ("any_shape",)


def kind_of(base):
    return base.get("kind", "conv")


def mod_of(base):
    return rm if kind_of(base) == "conv" else rr


def base_expect(base):
    return mod_of(base).EXPECT[base["id"]]


def segments(base):
    """[(chunk, first frame, end frame (both in the row's whole input), route tuple, has an incoming cache / state, record)]."""
    plan, chunks = base_expect(base)
    kind, out, t0 = kind_of(base), [], 0
    for j, T in enumerate(base["chunks"]):
        if plan == "generic":
            out.append((j, t0, t0 + T, ANY, bool(j or base.get("cache") or base.get("state")), None))
        elif kind == "gru":
            out.append((j, t0, t0 + T, rr.gru_tuple(chunks[j]), True, chunks[j]))
        else:
            tf = TILE if kind == "conv" else chunks[j][0][0]
            for i, rec in enumerate(chunks[j]):
                tup = rm.route_tuple(rec) if kind == "conv" else rr.fsmn_tuple(rec, i)
                has_in = bool(j or i or (base["cache"] if kind == "conv" else True))
                out.append((j, t0 + i * tf, t0 + min((i + 1) * tf, T), tup, has_in, rec))
        t0 += T
    return out


def issue_key(kind, tup):
    """The route keys of the coverage table: conv (family, nt, ctx, fast, split, persistent); GRU (family, nn, spw, time-chunked,
    pk, k2, nf_in_kernel, rounds > 1); FSMN (tile frames / 16, nt, u, head slices > 1, multi-tile)."""
    if tup == ANY or kind == "conv" or tup[0] == "padded":
        return tup
    return tup[:4] + tup[5:]


def tuple_key(kind, tup):
    """The error report's key of a route tuple (nonfinite_matrix/...)."""
    if tup == ANY:
        return f"{kind}/any_shape"
    if tup[0] == "padded":
        return f"{kind}/padded/{tup[1]}"
    if kind == "conv":
        return "conv/{}/nt{}_ctx{}_fast{}_split{}_pers{}".format(*tup)
    if kind == "gru":
        return "gru/{}/nn{}_spw{}_chunked{}_multi{}_pk{}_k2{}_nf{}_rounds{}".format(*tup)
    return "fsmn/maxnt{}_nt{}_u{}_slices{}_later{}_multi{}".format(*tup)


def universe():
    """{(kind, via, route tuple)}: what the poisoned matrix must reach."""
    need = set()
    for base in rm.ROWS + rr.ROWS:
        for _, _, _, tup, has_in, _ in segments(base):
            need.add((kind_of(base), "x", tup))
            if has_in:
                need.add((kind_of(base), "c", tup))
        if base_expect(base)[0] == "padded":       # every zero-padded model meets poison in its first call (NfCtx::skip_zero)
            need.add((kind_of(base), "x", ("padded", base["id"])))
    return need


def _upw(base):
    if kind_of(base) != "conv":
        return 1
    return max([int(rec.split()[5][3:]) for ch in base_expect(base)[1] for rec in ch] or [1])


def _persistent(base):
    return kind_of(base) == "conv" and any(tup != ANY and tup[5] for _, _, _, tup, _, _ in segments(base))


def utterances(base, rot):
    """The poisoned utterances of a row (see the module's docstring)."""
    B = base["B"]
    if B <= 2:
        return [rot % B]
    if _persistent(base):
        walk = list(range(0, B, rm.CUS))
        return sorted({walk[0], walk[len(walk) // 2], walk[-1], B - 1})
    if kind_of(base) == "gru" and B > 16:
        return sorted({0, 15, min(16, B - 1), B - 1})
    return [0, B - 1]


def _place(name, a, b, n):
    """(frame, feature) of a placement in the frames [a, b) of n features."""
    return {"first": (a, 0), "last": (b - 1, n - 1), "middle": ((a + b) // 2, n // 2)}[name]


def state_shape(base, cfg):
    return tuple(pack.cache_shape(pack.parse_config(cfg), base["B"]))


def _state_index(base, shape, u, k, rot):
    """The poisoned element of utterance u's incoming state (k: its number among the poisoned ones)."""
    pick = lambda n, w: {"first": 0, "last": n - 1, "middle": n // 2}[PLACES[w % 3]]        # noqa: E731
    w = rot + k
    if kind_of(base) == "gru":                                   # (L, B, H): the last / the first layer alternately
        return ((shape[0] - 1, 0)[k % 2], u, pick(shape[2], w))
    return (u,) + tuple(pick(n, w) for n in shape[1:])           # conv (B, C, P), FSMN (B, D, P, L)


def _derive_one(base, precision, plans, drot=0, number=0):
    """A derived row: the plans [(mode, segment)] of one base row in ONE run, each on utterances of its own (dealt in turn from
    utterances(base, rot)), so that a row that serves several routes is run once."""
    segs = segments(base)
    kind = kind_of(base)
    cfg = mod_of(base).row_config(base)
    idim = cfg["input_dim"]
    tag = "+".join(f"{m}{s}" for m, s in plans) + (f"#{number}" if number else "")
    rid = f"{base['id']}@{precision}/{tag}"
    rot = zlib.crc32(rid.encode()) % 15 + drot                   # the row's rotation: a function of its name, not of its neighbours
    U = utterances(base, rot)
    assert 1 <= len(plans) <= len(U), (base["id"], plans, U)
    poison, claims, k = [], [], 0
    for i, (mode, s) in enumerate(plans):
        mine = U[i::len(plans)]
        j, a, b, tup, _, rec = segs[s]
        later = s + 1 < len(segs)
        if mode == "x":
            lo = a
            if kind == "gru" and rec is not None and rec[3] and b - a > rec[3]:
                lo = a + rec[3] * ((b - a - 1) // rec[3])            # time-chunked gru_f16: the last time chunk
            for n, u in enumerate(mine):
                name = "last" if later and n == 0 else PLACES[(rot + k) % 3]
                t, f = _place(name, lo, b, idim)
                poison.append(("x", u, t, f, (rot + k) % 5))
                k += 1
        else:
            shape = state_shape(base, cfg)
            for u in mine:
                poison.append(("c", _state_index(base, shape, u, k, rot), (rot + k) % 5))
                k += 1
        # what the plan claims to reach, and in which utterances
        claims.append((s, mode, mine))
        if kind == "gru":
            claims += [(q, "c", mine) for q in range(s + 1, len(segs))]   # a non-finite GRU state stays one
        elif later and mode == "x":
            claims.append((s + 1, "c", mine))
    zero = any(m == "c" for m, _ in plans) and not (base.get("cache") or base.get("state"))
    return dict(id=rid, base=base, kind=kind, precision=precision, plans=list(plans), poison=poison,
                bad=sorted(U), claims=claims, zero_state=zero)


def _candidates(base):
    """(mode, segment) plans of a base row, each with the {(kind, via, tuple)} it reaches."""
    segs = segments(base)
    kind = kind_of(base)
    out = []
    for s, (j, a, b, tup, has_in, _) in enumerate(segs):
        got = {(kind, "x", tup)}
        if kind == "gru":
            got |= {(kind, "c", t[3]) for t in segs[s + 1:]}
        elif s + 1 < len(segs):
            got.add((kind, "c", segs[s + 1][3]))
        if s == 0 and base_expect(base)[0] == "padded":
            got.add((kind, "x", ("padded", base["id"])))
        out.append(("x", s, got))
    if kind != "conv" or base["cache"]:
        got = {(kind, "c", segs[0][3])}
        if kind == "gru":
            got |= {(kind, "c", t[3]) for t in segs[1:]}
        out.append(("c", 0, got))
    return out


# Rows whose poison was MOVED (a rotation offset: other placements and values) or that were reseeded (GRU / FSMN rows only: other
# weights and inputs than the base row's): the float32 oracle of the first placement did not stay under TIGHT_K / 2 of the float64
# oracle, or no weight matrix of the row was visible enough on what stayed finite (tests/test_nonfinite_matrix.py: reference
# side, value side).  The bar is never what moves.  {derived row id: (rotation offset, reseed offset)}
MOVED = {
    "fsmn/ctc2599/B1/T64_cache@default/c0": (0, 3),             # float32 oracle at 0.50 of the bar -> 0.35
    "fsmn/ctc2599/B1/T64_cache@default/x0#1": (1, 0),           # 1.44 (the first frame: 15 finite frames set the scales) -> 0.08
    "fsmn/ctc300/B1/T130_cache@default/c0": (1, 1),             # 1.66 -> 0.34
    "fsmn/ctc300_lin384/B1/T50_cache@default/c0": (0, 1),       # 0.46 -> 0.20
    "gru/f16/chunked/B1/T33@default/c0": (0, 1),                # 0.76 (one utterance: 128 finite state values, each its own scale) -> 0.09
    "gru/pipe/spw1/nf1/k2_1/B4/T15@default/c0+x0": (1, 0),      # nothing finite left (one layer, the first frame) -> the last frame
    "gru/pipe/spw16/nf1/k2_1/B1/T98@default/c0": (0, 1),        # 1.24 (as above) -> 0.29
}


def _cost(base):
    return base["B"] * sum(base["chunks"])


def plan_rank(base, mode, s):
    """The order in which plans are preferred: one that keeps the earlier chunks of a B = 1 row a clean stream before one that
    does not, a GRU row with an identity head before one whose sigmoid hides the values (rr's docstring), then the cheaper base
    row (B x frames), then by name."""
    early = base["B"] == 1 and segments(base)[s][0] != len(base["chunks"]) - 1
    hidden = kind_of(base) == "gru" and not rr.is_identity(base)
    return (early, hidden, _cost(base), base["id"], mode, s)


def derive():
    """The derived rows.  For every member of universe() the cheapest base row with a plan that reaches it (a plan that poisons an
    earlier chunk of a B = 1 row ranks behind every plan that does not; a GRU row with a sigmoid head behind every identity
    row); cheap plans first, and what a chosen plan reaches on the way counts.  The plans of one base row are merged into one
    run (_derive_one).  Then, for every family with a one-fp16-product variant, the cheapest row whose FIRST segment runs it,
    poisoned there, under precision f16 (the repair is IEEE f32 whatever was asked)."""
    bases = sorted(rm.ROWS + rr.ROWS, key=lambda r: (_cost(r), r["id"]))
    cands = [(base, mode, s, got) for base in bases for mode, s, got in _candidates(base)]

    best = {need: min((c for c in cands if need in c[3]), key=lambda c: plan_rank(*c[:3])) for need in universe()}
    chosen, covered = {}, set()
    for need in sorted(best, key=lambda n: (plan_rank(*best[n][:3]), repr(n))):     # cheap plans first; what they reach on the way counts
        if need in covered:
            continue
        base, mode, s, got = best[need]
        chosen[(base["id"], mode, s)] = base
        covered |= got
    by_base = {}
    for (_, mode, s), base in sorted(chosen.items(), key=lambda kv: (kv[1]["id"], kv[0][2], kv[0][1])):
        by_base.setdefault(base["id"], (base, []))[1].append((mode, s))
    rows = []
    for _, (base, plans) in sorted(by_base.items()):
        number = 0
        while plans:
            n = len(utterances(base, 0))
            row = _derive_one(base, base["precision"], plans[:n], 0, number)
            if row["id"] in MOVED:
                drot, dseed = MOVED[row["id"]]
                moved = dict(base, reseed=base["reseed"] + dseed) if dseed else base
                row = _derive_one(moved, base["precision"], plans[:n], drot, number)
            rows.append(row)
            plans, number = plans[n:], number + 1
    for fam in rm.ONE_PRODUCT:                   # the f16 reruns: poisoned from the first call on, so that the repair starts from exact inputs
        fit = [b for b in bases if kind_of(b) == "conv" and rm.is_split_row(b) and segments(b)[0][3][0] == fam]
        rows.append(_derive_one(min(fit, key=lambda b: (_cost(b), b["id"])), "f16", [("x", 0)]))
    return rows


ROWS = derive()
BY_ID = {r["id"]: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


def reached(rows=None):
    """{(kind, via, tuple)} the derived rows claim (rows of the matrices' own precision: the f16 reruns count for nothing)."""
    got = set()
    for row in rows or ROWS:
        if row["precision"] != row["base"]["precision"]:
            continue
        segs = segments(row["base"])
        got |= {(row["kind"], via, segs[s][3]) for s, via, _ in row["claims"]}
        if base_expect(row["base"])[0] == "padded" and ("x", 0) in row["plans"]:
            got.add((row["kind"], "x", ("padded", row["base"]["id"])))
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# a derived row's model and inputs
def row_case(row):
    """(cfg, weights, poisoned x, poisoned incoming state or None, clean x, clean incoming state or None)."""
    base, m = row["base"], mod_of(row["base"])
    cfg = m.row_config(base)
    cfg["_precision"] = row["precision"]
    sd = m.row_weights(base, cfg)
    x0 = m.row_input(base, cfg)
    c0 = rm.row_cache(base, cfg) if row["kind"] == "conv" else rr.row_state(base, cfg)
    if c0 is None and row["zero_state"]:
        c0 = np.zeros(state_shape(base, cfg), np.float32)
    x, c = x0.copy(), None if c0 is None else c0.copy()
    for p in row["poison"]:
        if p[0] == "x":
            x[p[1], p[2], p[3]] = VALUES[p[4]]
        else:
            c[p[1]] = VALUES[p[2]]
    return cfg, sd, x, c, x0, c0


def expect(row, lib=None):
    """(plan, the predicted trace of every chunk): the base row's; an f16 rerun's comes from route.h (lib: the hooks library)."""
    base = row["base"]
    if row["precision"] == base["precision"]:
        return base_expect(base)
    return rm.predict(lib, base, row["precision"])


def take(kind, state, idx):
    """Utterances idx of a state / cache (the GRU's is (L, B, H))."""
    if state is None:
        return None
    return np.ascontiguousarray(state[:, idx] if kind == "gru" else state[idx])


def utt_mask(kind, shape, idx, state=False):
    """A boolean mask of `shape` that is True in the utterances idx."""
    m = np.zeros(shape, bool)
    if state and kind == "gru":
        m[:, idx] = True
    else:
        m[idx] = True
    return m


def reference(cfg, sd, x, c0, chunks, dtype, forward=None):
    """The oracle chunk by chunk with the state carried -> ([y of every chunk], [state after every chunk])."""
    from oracle import kws_oracle
    fwd = forward or kws_oracle.forward
    ys, cs, c, t = [], [], c0, 0
    with np.errstate(all="ignore"):
        for n in chunks:
            y, c = fwd(cfg, sd, x[:, t:t + n], c, dtype=dtype)
            ys.append(y)
            cs.append(c)
            t += n
    return ys, cs


def segment_chunks(row):
    """The row's chunks cut further at the segment boundaries (the oracle in these pieces = the oracle in the row's chunks)."""
    return [b - a for _, a, b, _, _, _ in segments(row["base"])]


def calibration_subset(row, n=6):
    """At most n utterances of a row for the CPU calibration (the bar is per element): the poisoned ones (four at the most), then
    clean ones -- two where the row has them: a channel's scale is taken over the finite values, and a subset with a single
    clean utterance would hold that one to its own magnitude element by element."""
    B, bad = row["base"]["B"], row["bad"]
    return sorted(list(bad) + [u for u in range(B) if u not in bad][:max(0, min(n, B) - len(bad))])


def nothing_to_see(row):
    """Rows whose poisoned utterances keep NOTHING finite that a weight has touched, whatever the placement: every plan either
    poisons the state of a one-layer GRU (a NaN state never leaves) or the only frame of a one-frame call (the output is that
    frame's; what stays finite in the returned cache is copied from the incoming one).  On such a row the device is checked by
    classes alone; the GPU test says so in the error report (nonfinite_matrix/classes_only/...)."""
    segs = segments(row["base"])
    one_layer = row["kind"] == "gru" and mod_of(row["base"]).row_config(row["base"])["backbone"]["num_layers"] == 1
    return all((mode == "c" and one_layer) or (mode == "x" and segs[s][2] - segs[s][1] == 1 and (one_layer or s == len(segs) - 1))
               for mode, s in row["plans"])


def hooks():
    return rm.type_hooks(C.CDLL(rm.hooks_path()))
