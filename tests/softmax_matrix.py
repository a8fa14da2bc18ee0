"""The matrix of the two softmax kernels -- softmax_rows_kernel (forward_softmax, reached through the hooks library's
wekws_hip_debug_softmax_rows) and softmax_topk_kernel (wekws_hip_softmax_topk) -- against the float64 oracle of
oracle/topk_oracle.py in softmax_units at K_SOFTMAX (tests/helpers.py).  Importable without a GPU.  Shared by
  * tests/test_softmax_matrix.py (CPU): the matrix is what it says it is, the calibration of K_SOFTMAX from two float32 evaluations,
    the negative controls (emulations of the kernels' order of operations, kernel_order below);
  * tests/tools/softmax_matrix_cases.py -> tests/test_hip_softmax_f64.py (GPU): every row through both kernels.
A row is (id, rows, K, law, k): `rows` rows of K logits drawn by `law`, and the k of the top-k launch.  Ids are law/K<K>_r<rows>.

Both kernels read a row the same way: lane l of the row's wave takes the 16-byte vectors at 4 l + 256 i, i = 0, 1, ..., below
K4 = K & ~3, then lane l < K - K4 takes the tail element K4 + l.  The class counts and the placements below follow from that."""
from collections import namedtuple

import numpy as np

Row = namedtuple("Row", "id rows K law k")

# K < 4 (the tail path alone); every remainder K % 4 on both sides of the 256-element lane stride; odd K (rows only dword
# aligned); below, at and above the wave width; the CTC vocabulary; several strides per lane
KS = (1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 127, 255, 256, 257, 258, 259, 1023, 1024, 1027, 2599, 5000, 10007)
ROW_COUNTS = (1, 3, 4, 5, 66)          # four rows per workgroup: 66 is 16 workgroups and a half
MANY = 66                              # (the gauss3 rows carry it for every K; the other laws cycle through the small counts)
KTOP = tuple(range(1, 9))              # every k is its own template instantiation

# Gaussian rows are N(0, 1) clipped to +-3, times the spread: the widest row then spans 72 (spread 12), its smallest posterior is
# above exp(-72) / K >= exp(-81.3) > 2^-126 = exp(-87.3), so no row but the `deep` ones has a posterior below float32's normal range.
CLIP = 3.0
FINITE_LAWS = ("gauss0.1", "gauss3", "gauss12", "offset+1e4", "offset-1e4", "ascending", "descending", "max_last_vector", "max_tail",
               "max_tied", "deep")
MASK_LAWS = ("mask_index0", "mask_lane_first", "mask_lane_vector", "mask_tail", "mask_first256", "mask_all_but_one", "mask_all")
POISON_LAWS = ("nan_one", "posinf_one", "nan_lane")
NAN_ROW_LAWS = ("mask_all",) + POISON_LAWS                      # the oracle's posteriors are NaN in every class
DEEP_SHARE = 8                                                   # `deep`: at most 1 / 8 of a row's classes below the normal range


def law_fits(law, K):
    """Does the law have a meaning at this class count?"""
    K4, tail = K & ~3, K % 4
    return {"max_last_vector": K4 > 0, "max_tail": tail > 0, "max_tied": K >= 2, "deep": K >= DEEP_SHARE,
            "mask_index0": K >= 2, "mask_lane_first": K >= 8, "mask_lane_vector": K >= 5, "mask_tail": tail > 0 and K >= 2,
            "mask_first256": 256 < K <= 300, "mask_all_but_one": K >= 2, "nan_lane": K == 300}.get(law, True)


def poison_index(K):
    return (K * 5) // 7


def masked_indices(law, K):
    """The classes a mask law sets to -Inf."""
    K4 = K & ~3
    if law == "mask_index0":
        return [0]
    if law == "mask_lane_first":                                  # the first element every lane sees in the vector loop
        return list(range(0, min(K4, 256), 4))
    if law == "mask_lane_vector":                                 # a lane's whole first 16-byte load: lane 0, and lane 7 where it has one
        return [0, 1, 2, 3] + ([28, 29, 30, 31] if K4 >= 32 else [])
    if law == "mask_tail":                                        # the tail remainder (K < 4: the last class, the row is all tail)
        return list(range(K4, K)) if K4 else [K - 1]
    if law == "mask_first256":                                    # one whole stride: the lanes without a second vector see -Inf alone
        return list(range(256))
    if law == "mask_all_but_one":
        return [i for i in range(K) if i != poison_index(K)]
    if law == "mask_all":
        return list(range(K))
    raise KeyError(law)


def _gauss(g, rows, K, spread):
    return np.clip(g.standard_normal((rows, K)), -CLIP, CLIP) * spread


def row_logits(row):
    """(rows, K) float32, seeded by the row's id alone."""
    _, rows, K, law, _ = row
    g = np.random.default_rng([0x50F7, rows, K, sum(map(ord, law))])
    K4, r = K & ~3, np.arange(rows)
    if law.startswith("gauss"):
        x = _gauss(g, rows, K, float(law[5:]))
    elif law.startswith("offset"):
        x = _gauss(g, rows, K, 3.0) + float(law[6:])
    elif law in ("ascending", "descending"):                      # ascending: every element a lane meets is a new maximum
        x = np.linspace(-20.0, 20.0, K)[None, :] + g.uniform(-1, 1, (rows, 1))
        x = x[:, ::-1] if law == "descending" else x
    else:
        x = _gauss(g, rows, K, 3.0)
    x = np.ascontiguousarray(x, np.float32)
    top = x.max(axis=1) + np.float32(2.0)
    if law == "max_last_vector":
        x[r, K4 - 1 - r % 4] = top
    elif law == "max_tail":
        x[r, K4 + r % (K % 4)] = top
    elif law == "max_tied":                                       # exact ties of the maximum: first, middle and last class
        for i in {0, K // 2, K - 1}:
            x[r, i] = top
    elif law == "deep":                                           # 1 / 8 of the classes 100 .. 120 below the maximum
        n = K // DEEP_SHARE
        for i in range(rows):
            x[i, g.choice(K, n, replace=False)] = x[i].max() - g.uniform(100.0, 120.0, n).astype(np.float32)
    elif law in MASK_LAWS:
        x[:, masked_indices(law, K)] = -np.inf
    elif law == "nan_one":
        x[:, poison_index(K)] = np.nan
    elif law == "posinf_one":
        x[:, poison_index(K)] = np.inf
    elif law == "nan_lane":                                       # the only vector lane 20 of a 300-class row reads
        x[:, 80:84] = np.nan
    return x


def _rows():
    out, n = [], 0
    for law in FINITE_LAWS + MASK_LAWS + POISON_LAWS:
        for K in KS + (300,):
            if K == 300 and law not in ("mask_first256", "nan_lane", "gauss12"):
                continue
            if not law_fits(law, K):
                continue
            rows = MANY if law == "gauss3" else ROW_COUNTS[n % 4]
            out.append(Row(f"{law}/K{K}_r{rows}", rows, K, law, KTOP[n % 8]))
            n += 1
    return out


ROWS = _rows()
IDS = [r.id for r in ROWS]
assert len(set(IDS)) == len(IDS)
BY_ID = {r.id: r for r in ROWS}

# The negative controls (CPU emulations: kernel_order), each on the row named for it.
CONTROL_ROWS = {"tail_dropped": "gauss0.1/K2599",       # the K % 4 tail classes left out of the denominator: a flat CTC-sized row
                "lane_unscaled": "gauss12/K300",        # one lane's partial sum added without its rescale to the row maximum
                "coarse_argument": "gauss0.1/K2599"}    # the exponent's argument on a 2^-16 grid


def control_row(name):
    return next(r for r in ROWS if r.id.startswith(CONTROL_ROWS[name] + "_"))


# ---------------------------------------------------------------------------------------------------------------------
# float32 evaluations (the calibration's two sides are in tests/test_softmax_matrix.py) and the kernels' order, emulated
def _exp32(a, grid=None):
    """exp of a float32 array, correctly rounded to float32 (grid: the argument first rounded to multiples of it)."""
    a = a.astype(np.float64)
    if grid:
        a = np.round(a / grid) * grid
    with np.errstate(all="ignore"):
        return np.exp(a).astype(np.float32)


def two_pass_f32(x):
    """The plain float32 softmax: maximum, exp(x - m), numpy's (pairwise) sum, one division per element."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        e = np.exp(x - x.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True, dtype=np.float32)


def serial_f32(x):
    """The same with a strictly serial single-accumulator float32 sum (informational: correct, and outside the bar by design)."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        e = np.exp(x - x.max(axis=-1, keepdims=True))
        return e / np.cumsum(e, axis=-1, dtype=np.float32)[..., -1:]


def kernel_order(x, drop_tail=False, unscaled_lane=False, grid=None):
    """softmax_rows_kernel's order of float32 operations on (rows, K), with a correctly rounded exp in place of the hardware's:
    per lane the online (maximum, rescaled sum) over its strided vectors and its tail element, the maximum over the 64 lanes, every
    lane's sum rescaled to it, a butterfly sum, one reciprocal, exp(x - m) * inv.  The defects of the negative controls:
    drop_tail: the tail classes are left out of the denominator; unscaled_lane: the lane after the one that holds the maximum adds
    its sum without the rescale; grid: the exponent's argument is rounded to multiples of it."""
    x = np.asarray(x, np.float32)
    R, K = x.shape
    K4 = K & ~3
    lane = np.arange(64)
    mx = np.full((R, 64), -np.inf, np.float32)
    s = np.zeros((R, 64), np.float32)

    def take(v, on):
        nonlocal mx, s
        with np.errstate(all="ignore"):
            on = on & (v != -np.inf)
            up = on & (v > mx)
            s = np.where(up, s * _exp32(mx - v, grid), s)
            mx = np.where(up, v, mx)
            s = np.where(on, s + _exp32(v - mx, grid), s)

    for base in range(0, K4, 256):
        for j in range(4):
            i = base + 4 * lane + j
            take(x[:, np.minimum(i, K - 1)], np.broadcast_to(i < K4, (R, 64)))
    if not drop_tail:
        i = K4 + lane
        take(x[:, np.minimum(i, K - 1)], np.broadcast_to(i < K, (R, 64)))
    with np.errstate(all="ignore"):
        gm = mx.max(axis=1, keepdims=True)
        gs = np.where(mx == -np.inf, s, s * _exp32(mx - gm, grid))
        if unscaled_lane:
            bad = (mx.argmax(axis=1) + 1) % 64
            gs[np.arange(R), bad] = s[np.arange(R), bad]
        for off in (32, 16, 8, 4, 2, 1):
            gs = gs + gs[:, lane ^ off]
        inv = np.float32(1.0) / gs[:, :1]
        return _exp32(x - gm, grid) * inv
