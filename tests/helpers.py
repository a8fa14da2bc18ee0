"""Shared by the CPU and GPU tests: seeded weights / inputs for a golden case (no reference import)."""
import numpy as np

from tests.golden.cases import CASES, case_config, case_in_cache, case_input  # noqa: F401
from tests.golden.nonfinite_cases import classify as value_classes  # 0 finite, 1 NaN (any encoding), 2 +Inf, 3 -Inf
from wekws_amd import pack
from wekws_amd.utils import synth


def case_weights(case):
    cfg = case_config(case)
    sd = synth.synth_state_dict(pack.model_spec(cfg), case["wseed"])
    return cfg, sd


def by_name(name):
    for c in CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


def max_abs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) if np.size(a) else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# A forward-laid-out FlatBuffers writer, just enough to hand-build an ORT-format image for the .ort reader test
# (uoffsets point forward from the referencing slot, so parents are written before their children).
class _FlatWriter:
    def __init__(self, ident=b"ORTM"):
        import struct
        self.s = struct
        self.b = bytearray(4) + ident

    def _align(self, n):
        while len(self.b) % n:
            self.b.append(0)

    def table(self, fields):
        """fields: [(slot, fmt | 'ref', value | emitter)] -> position of the table."""
        s = self.s
        nslots = max(f[0] for f in fields) + 1
        offs, cur = {}, 4
        for slot, fmt, _ in fields:
            size = 4 if fmt == "ref" else s.calcsize(fmt)
            cur = (cur + size - 1) // size * size
            offs[slot] = cur
            cur += size
        self._align(8)
        vt = len(self.b)
        self.b += s.pack("<HH", 4 + 2 * nslots, cur) + b"".join(s.pack("<H", offs.get(i, 0)) for i in range(nslots))
        self._align(8)
        t = len(self.b)
        self.b += s.pack("<i", t - vt) + bytes(cur - 4)
        for slot, fmt, val in fields:
            if fmt != "ref":
                s.pack_into("<" + fmt, self.b, t + offs[slot], val)
        for slot, fmt, val in fields:
            if fmt == "ref":
                child = val()
                s.pack_into("<I", self.b, t + offs[slot], child - (t + offs[slot]))
        return t

    def string(self, text):
        self._align(4)
        p = len(self.b)
        self.b += self.s.pack("<I", len(text)) + text.encode() + b"\0"
        return p

    def scalars(self, fmt, vals):
        size = self.s.calcsize(fmt)
        while (len(self.b) + 4) % max(size, 4):
            self.b.append(0)
        p = len(self.b)
        self.b += self.s.pack("<I", len(vals)) + b"".join(self.s.pack("<" + fmt, v) for v in vals)
        return p

    def refs(self, emitters):
        self._align(4)
        p = len(self.b)
        self.b += self.s.pack("<I", len(emitters)) + bytes(4 * len(emitters))
        for i, e in enumerate(emitters):
            slot = p + 4 + 4 * i
            self.s.pack_into("<I", self.b, slot, e() - slot)
        return p

    def finish(self, root):
        self.s.pack_into("<I", self.b, 0, root)
        return bytes(self.b)


def build_tiny_ort():
    """InferenceSession{ort_version, model{opset, graph{1 initializer, 1 node with f / ints / s attributes, inputs,
    outputs}, metadata_props}} in the slot layout of ort.fbs (ORT 1.12) -> (bytes, the initializer's values)."""
    w = _FlatWriter()
    S = lambda text: (lambda: w.string(text))                                         # noqa: E731
    SV = lambda texts: (lambda: w.refs([S(t) for t in texts]))                        # noqa: E731
    T = lambda fields: (lambda: w.table(fields))                                      # noqa: E731
    vals = np.arange(6, dtype=np.float32).reshape(2, 3) - 2.5
    tensor = T([(0, "ref", S("w")), (2, "ref", lambda: w.scalars("q", [2, 3])), (3, "i", 1),
                (4, "ref", lambda: w.scalars("B", list(vals.tobytes())))])
    attrs = [T([(0, "ref", S("alpha")), (2, "i", 1), (3, "f", 0.5)]),
             T([(0, "ref", S("axes")), (2, "i", 7), (9, "ref", lambda: w.scalars("q", [1, 2]))]),
             T([(0, "ref", S("mode")), (2, "i", 3), (5, "ref", S("x"))])]
    node = T([(0, "ref", S("n0")), (4, "I", 0), (5, "ref", S("Relu")), (8, "ref", SV(["input"])),
              (9, "ref", SV(["output"])), (10, "ref", lambda: w.refs(attrs))])
    graph = T([(0, "ref", lambda: w.refs([tensor])), (2, "ref", lambda: w.refs([node])), (5, "ref", SV(["input", "w"])),
               (6, "ref", SV(["output"]))])
    model = T([(0, "q", 7), (1, "ref", lambda: w.refs([T([(0, "ref", S("")), (1, "q", 13)])])), (7, "ref", graph),
               (9, "ref", lambda: w.refs([T([(0, "ref", S("cache_dim")), (1, "ref", S("4"))])]))])
    root = w.table([(0, "ref", S("1.12.0")), (1, "ref", model)])
    return w.finish(root), vals


def random_model_config(rng):
    """A configuration init_model accepts (kws_model.py:97-214), drawn around the thresholds between the specialised kernels and
    the any-shape path: hidden sizes on and off the built widths, kernel sizes, depths, feature widths, class counts, heads."""
    kind = str(rng.choice(["ds", "tcn", "mdtc", "gru"]))
    idim = int(rng.choice([40, 80, 23, 64]))
    odim = int(rng.choice([1, 2, 3, 12, 20]))
    cfg = {"input_dim": idim, "output_dim": odim, "preprocessing": {"type": "linear"}}
    if kind in ("ds", "tcn"):
        h = int(rng.choice([16, 32, 64, 96, 128, 256, 256, 320] if kind == "ds" else [16, 32, 64, 80, 128]))
        cfg["hidden_dim"] = h
        cfg["backbone"] = {"type": "tcn", "ds": kind == "ds", "num_layers": int(rng.integers(1, 8)),
                           "kernel_size": int(rng.choice([3, 5, 8, 8, 8, 9])), "dropout": 0.1}
    elif kind == "mdtc":
        h = int(rng.choice([16, 32, 48, 64, 64, 128, 160]))
        cfg["hidden_dim"] = h
        cfg["backbone"] = {"type": "mdtc", "num_stack": int(rng.integers(1, 6)), "stack_size": int(rng.choice([1, 2, 3, 4, 4, 5, 6])),
                           "kernel_size": int(rng.choice([3, 5, 5, 5, 7])), "hidden_dim": h, "causal": True}
    else:
        cfg["hidden_dim"] = int(rng.choice([32, 64, 128, 128, 160]))
        cfg["backbone"] = {"type": "gru", "num_layers": int(rng.integers(1, 6))}
    head = str(rng.choice(["linear", "linear", "global", "last"]))
    if head != "linear":
        cfg["classifier"] = {"type": head, "dropout": 0.5}
    if rng.integers(0, 4) == 0:
        cfg["activation"] = {"type": "identity"}
    if rng.integers(0, 3) == 0:                       # GlobalCMVN in front (cmvn.py:45-48), with or without the variance
        cfg["cmvn"] = {"norm_var": bool(rng.integers(0, 2))}
        cfg["_cmvn"] = True                          # (statistics come as buffers of the state dict, not from a cmvn_file)
    if rng.integers(0, 6) == 0:                       # NoSubsampling (subsampling.py:35-36): features ARE the hidden tile
        cfg["preprocessing"] = {"type": "none"}
        cfg["input_dim"] = cfg["hidden_dim"]
    return cfg, head


def random_config_spec(cfg):
    """State-dict spec of a random_model_config model as the reference builds it for the live comparison: init_model without
    the CMVN, the GlobalCMVN assigned afterwards, so its two buffers come last (the order the seeded weight stream follows)."""
    spec = pack.model_spec(cfg)
    cmvn = [s for s in spec if s[0].startswith("global_cmvn.")]
    return [s for s in spec if not s[0].startswith("global_cmvn.")] + cmvn


# ---------------------------------------------------------------------------------------------------------------------
# The tight bar: a result against the FLOAT64 evaluation of the same function (oracle/kws_oracle.py, dtype=np.float64).
#   * posteriors / probabilities (sigmoid or softmax outputs): absolute error;
#   * logits, pooled heads and caches: per channel, |got - ref| <= k * S_c with S_c = max(max over the other axes of |ref| in
#     channel c, 2^-10 * max|ref|) -- a channel that is small next to the others is held to its own magnitude, not to the
#     largest element of the tensor.
# One k for every exact-f32 and split-fp16 (F16X3, three fp16 products) route.  The single-fp16-product routes (precision F16)
# keep their own comparison (F16_TOL against folded_oracle's fp16-operand emulation).  TIGHT_K is calibrated from both sides:
#   * CPU, every row of tests/route_matrix.py (tests/test_route.py::test_tight_bar_separates_f32_from_one_fp16_product): the
#     float32 oracle reaches 6.4e-6 (the 2599-class CTC head, whose logits cancel in some classes -- why 2^-17 is too tight for a
#     correct float32 evaluation), ATen float32 likewise; both fp16 emulations miss by 2.9e-4 at least;
#   * GPU, every row (tests/test_hip_route_matrix.py): at most 4.0e-6 (ds256_mm, the CTC heads), 9.7e-7 on every other family;
#     every one-fp16-product control at least 12x the bar.
# 2^-15 (3.05e-5): 7.6x the largest measured kernel error, 4.8x the float32 oracle's, 9.6x below the fp16 emulations.
# GRU and FSMN (tests/route_matrix_rnn.py: 55 GRU + 29 FSMN rows over every route tuple of select_gru_route / select_fsmn_route;
# every chunk's output compared on its own, the GRU's state after every chunk, the FSMN's final cache; four named CTC-head rows
# that carry a stream over short calls take each class's scale over the whole stream -- the reason stands beside them):
#   * CPU, every row at <= 4 utterances (tests/test_route.py::test_tight_bar_holds_f32_and_rejects_one_rounded_matrix): the
#     float32 oracle and ATen float32 reach 5.4e-6 on the GRU rows (ATen, the 5-layer any-shape row; 4.1e-6 on the kernels'
#     rows) and the float32 oracle 5.4e-6 on the FSMN rows (the first call of a CTC-head stream; 3.5e-6 otherwise); the least
#     visible SINGLE weight matrix rounded to fp16 misses the bar by 2.48x (GRU: the classifier, here of the hidden-160 model)
#     and 2.42x (FSMN: a layer's affine transform), most matrices by 3 .. 30x;
#   * GPU (tests/test_hip_route_gru_fsmn.py), at the full batch, measured on the 59 single-chunk rows (a multi-chunk row's
#     figures are in the error report of a GPU run, route_matrix/gru/... and route_matrix/fsmn/...): GRU at most 3.9e-6 (a
#     state channel of a two-stream row), FSMN at most 2.4e-6 (the 2599-class head); the rounded-matrix control misses the bar
#     on each of their 40 control rows, by 1.78x at least for the GRU (a full batch raises the channels' scales above those
#     of the 4-utterance CPU case) and 2.41x for FSMN.
# Non-finite inputs (tests/nonfinite_matrix.py: 171 rows DERIVED from the two matrices, NaN / +-Inf in the features or in the
# incoming cache / state of every route tuple -- conv 92 / 92, GRU 31 / 31, FSMN 22 / 22 by the coarse keys of nm.issue_key, plus
# the padded and any-shape plans; masked_tight_error: classes first, then the bar on the finite values with S_c over the finite
# reference values).  Calibrated on the CPU from three sides (tests/test_nonfinite_matrix.py), at the poisoned utterances plus two
# clean ones of every row:
#   * reference side: the float32 oracle has the float64 oracle's classes on every row and reaches 0.35 of the bar (FSMN, the
#     2599-class head from a poisoned cache at B = 1), 0.30 (conv) and 0.29 (GRU); on the 33 golden cases 4.5e-6 = 0.15 of the
#     bar (mdtc_small_last12/full).  Seven rows were moved or reseeded for it (nm.MOVED: one utterance whose few finite frames
#     set every channel's scale is held to its own magnitude element by element); the bar did not move.
#   * defect side, each a CLASS mismatch: the oracle with an fmax ReLU (relu(NaN) = 0: a missed detection) on each of the 125
#     rows where a NaN meets a ReLU; the oracle on zero-padded weights (0 x NaN: skip_zero off) on the row whose KERNEL SIZE is
#     padded -- where only the width is padded it cannot differ in what the caller sees, which the test asserts too --;
#     NoSubsampling through the full matrix product (0 x Inf) on the golden case without a subsampling layer.
#   * value side: on the finite values of the poisoned utterances ALONE, the most visible single weight matrix rounded to fp16
#     misses the bar by 8.0 x (conv) / 3.1 x (FSMN) / 2.2 x (GRU) at the least, CONTROL_MARGIN = 1.5 asked; six rows keep nothing
#     finite that a weight has touched (a poisoned state of a one-layer GRU, the only frame of a one-frame call) and are
#     exempt by that rule, not by name.
# GPU (tests/test_hip_nonfinite_matrix.py), all 171 rows, repaired and clean parts alike: conv at most 7.6e-6 (the repaired
# utterances 3.8e-6), FSMN 1.27e-5 (the 2599-class head at B = 1, poisoned cache), GRU 1.62e-5 = 0.53 of the bar (h0 poisoned in
# the last layer at B = 1: the first layer's 128 finite state values, each its own scale); the six stress rows at most 1.7e-6;
# the f16 reruns' fast path at 0.01 of its 2e-2.  Per route in the error report of a GPU run under nonfinite_matrix/...
TIGHT_K = 2.0 ** -15
F16_TOL = 5e-4
CHANNEL_FLOOR = 2.0 ** -10


def tight_error(got, ref, axis=None):
    """max |got - ref| / S_c (axis: the channel axis) or max |got - ref| (axis None: probabilities), in float64."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not got.size:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    d = np.abs(got - ref)
    if axis is None:
        return float(d.max())
    axis = axis % ref.ndim
    other = tuple(i for i in range(ref.ndim) if i != axis)
    a = np.abs(ref)
    s = np.maximum(a.max(axis=other, keepdims=True), CHANNEL_FLOOR * float(a.max()))
    s = np.where(s > 0, s, 1.0)
    return float((d / s).max())


def masked_tight_error(got, ref, axis=None, where=None, scale_ref=None):
    """tight_error for results that may hold NaN / +-Inf (non-finite inputs: tests/nonfinite_matrix.py).  Classes first: inf unless
    got and ref are finite / NaN / +Inf / -Inf at the same positions (where: a boolean mask of the positions that count, all of
    them by default).  Then max |got - ref| / S_c over the finite positions that count, S_c as in tight_error but taken over the
    FINITE values of the whole reference (scale_ref: of that tensor instead -- a stream's concatenated chunks), whatever `where`
    selects: a subset is held to the scales of the tensor it is part of."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    where = np.ones(ref.shape, bool) if where is None else np.broadcast_to(where, ref.shape)
    if not ref.size or not where.any():
        return 0.0
    cg, cr = value_classes(got), value_classes(ref)
    if not np.array_equal(cg[where], cr[where]):
        return float("inf")
    fin = (cr == 0) & where
    if not fin.any():
        return 0.0
    d = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, ref, 0.0)), 0.0)
    if axis is None:
        return float(d.max())
    sref = ref if scale_ref is None else np.asarray(scale_ref, np.float64)
    axis = axis % ref.ndim
    other = tuple(i for i in range(ref.ndim) if i != axis)
    a = np.where(np.isfinite(sref), np.abs(sref), 0.0)
    s = np.maximum(a.max(axis=other, keepdims=True), CHANNEL_FLOOR * float(a.max()))
    s = np.where(s > 0, s, 1.0)
    return float((d / s).max())


def y_axis(cfg, softmax=False):
    """The tight bar's channel axis of y: None for posteriors (sigmoid head, softmax), the class axis for logits / pooled heads."""
    from oracle.kws_oracle import classifier_kind
    _, act = classifier_kind(cfg)
    return None if (softmax or act == "sigmoid" or cfg.get("_exported_softmax")) else -1


def cache_axis(cfg):
    """The channel axis of the cache: (L, B, H) for the GRU, (B, C, P) / (B, D, P, L) for the conv backbones and FSMN."""
    return -1 if cfg["backbone"]["type"] == "gru" else 1


def oracle64(cfg, sd, x, in_cache=None, chunks=None, softmax=False):
    """The float64 oracle: one-shot or in chunks carrying the cache, like tests/test_hip_parity.py::run."""
    from oracle import kws_oracle
    if chunks:
        ys, c, t = [], in_cache, 0
        for n in chunks:
            y, c = kws_oracle.forward(cfg, sd, x[:, t:t + n], c, softmax=softmax, dtype=np.float64)
            ys.append(y)
            t += n
        return np.concatenate(ys, axis=1), c
    return kws_oracle.forward(cfg, sd, x, in_cache, softmax=softmax, dtype=np.float64)


def golden_oracle64(case, cfg, sd, x, c0):
    """The float64 oracle on a golden case (tests/golden/nonfinite_cases.py: chunks or one call, forward or forward_softmax)."""
    from oracle import kws_oracle
    with np.errstate(all="ignore"):
        if case.get("chunks"):
            return kws_oracle.forward_streaming(cfg, sd, x, case["chunks"], c0, dtype=np.float64)
        return kws_oracle.forward(cfg, sd, x, c0, softmax=case.get("softmax", False), dtype=np.float64)


def tight_errors(cfg, y, c, ry, rc, softmax=False):
    """(y error, cache error) under the tight bar; c / rc may be None."""
    ey = tight_error(y, ry, y_axis(cfg, softmax))
    ec = 0.0 if c is None else tight_error(c, rc, cache_axis(cfg))
    return ey, ec


# ---------------------------------------------------------------------------------------------------------------------
# The front end's tight bars: the fbank kernel and the DCT / lifter kernel against FLOAT64 evaluations of the same pipelines.
#
# K_FBANK, in the unit of oracle/fbank_oracle.py::fbank_units -- per mel bin b of a frame
#     u = |exp(got) - E| / (2 sqrt(E S) + S + eps E),   E = max(float64 mel energy, FLT_EPSILON),   eps = 2^-23,
#     S = (sum_k W[b, k]) eps^2 sum_i ((x_i - mean) win_i)^2
# (S: what float32 rounding of the DC-removed, windowed frame leaves in the bin as white noise; the denominator is the noise a
# correct float32 pipeline cannot avoid, in loud bins and in bins far below the frame's peak alike).  The rule: the smallest power
# of two at or above TWICE the largest u of a plain float32 restatement with exactly rounded twiddles (fbank_f32_exact: pocketfft
# on complex64, the rest in np.float32) -- the reference side's arithmetic, not the kernel's; the factor 2 is for the kernel's
# different but equivalent float32 order (radix-4 on a packed 256-point transform plus an untangle pass, always 512 points, a
# tree-summed mean, slot-wise mel sums).  tests/test_fbank_matrix.py::test_k_fbank_is_twice_the_float32_restatement asserts it.
#   * CPU, every row of tests/fbank_matrix.py and the first utterance of every case of framing_cases(0 .. 39):
#     fbank_f32_exact reaches 6.00 (8 kHz noise, 80 bins, Povey) -> 16; silence 3.63 (at the floor, through the same formula).  A log-mel
#     of 16 .. 32 stored as float32 is itself up to 8 of these units from the value it rounds (half an ulp of 20 is 9.5e-7 = 8 eps of
#     the energy): most of the 6.00 is the OUTPUT FORMAT, and the bar leaves a kernel the same again for its arithmetic.
#   * The reference ALGORITHM (oracle/fbank_oracle.c: recurrence sine table, radix-2, serial sums) reaches 8.64 on the same inputs:
#     inside the bar.  It measured up to 160 while fbank_f64 built its mel bank with numpy's float32 log: that is not libm's logf (the
#     two differ in the last bit for one argument in eight) and one ulp of a mel value moves a weight by tens of eps -- the bank
#     computed in double misses the bar for the same reason.  The arbiter takes the reference's bank from the C restatement now
#     (fbank_oracle.mel_bank), the same libm the host code of the kernel's table calls.  The old bars (1e-4 .. 1e-3 in the log
#     domain) were therefore not "sized to the reference's FFT noise": its FFT is as good as an exactly rounded one in this unit.
#   * Negative controls, CPU emulation on the control rows (noise at 80 bins in both windows, 8 kHz noise;
#     tests/test_fbank_matrix.py::test_control_emulations), each against the bar of 16 with CONTROL_MARGIN = 1.5:
#       one mel weight x (1 + 2^-12)           302 .. 407 in its bin, <= 4.5 elsewhere
#       the mel bank computed in double        32.5 .. 61.1                                     (kept: >= 1.5 x the bar)
#       twiddles on a 2^-18 grid               57.9 .. 64.9
#       twiddles by the float32 recurrence     4.1 .. 5.1: NOT a miss, and it cannot be one -- that table is 1.5 ulp of 1 off at
#                                              worst; the control is kept with the assertion that it stays inside the bar.
#   * GPU (tests/test_hip_fbank_f64.py, every row; per variant in the error report of a GPU run, fbank_f64/...): at most 6.55 (a sine
#     of the 3.3-round persistent row at 80 bins; 6.14 on the one-frame persistent row; 3.8 .. 5.6 on every other variant), noise
#     5.62, the int16 ramp 0.75, silence 3.63; the nine fuzz seeds of tests/test_hip_fbank.py at most 6.04, Mfcc's fbank stage 5.58.
#     The kernel sits where the float32 restatement does: 2.4 x below the bar.  Controls on the device, the three control rows:
#       one mel weight x (1 + 2^-12)           302.7 / 406.5 / 391.1 in its bin, <= 5.0 in every other bin
#       the mel bank computed in double        32.5 / 57.3 / 61.1
#       twiddles on a 2^-18 grid               57.8 / 45.4 / 44.4
#       twiddles by the float32 recurrence     5.9 / 4.8 / 5.0: inside the bar, as the emulation says
#     With the device library's logf in the kernel's last stage (v_log_f32 x ln 2: up to 2.31 ulp of its result = 35 eps of its
#     argument over 2^20 values in [e^-16, e^27], tools/probe/fbank_logf_probe.hip) the rows reached up to 26.7 (16.8 on the plain 40-bin row) and missed the bar:
#     the finding of this test.  fbank.hip.h::fb_logf (8.3 eps of the argument on the same values) is the fix.
#
# K_DCT, per element of dct_lifter in the unit eps |lifter_k| sum_j |M[j, k] x_j| (one rounding per product): the same rule.  A float32
# evaluation (kaldi_feats_oracle.dct_lifter_f32) reaches 3.24 over tests/fbank_matrix.py::DCT_SHAPES (every square shape 1 .. 128)
# -> 8; one matrix entry x (1 + 2^-12), the largest of its column, shows as 15.1 at the least (128 x 128) in that column over three
# rows or more.  The kernel computes its matrix itself (no table to perturb on the device), so this control is a CPU emulation alone.
# GPU (tests/test_hip_mfcc_f64.py): at most 1.89 (the tail of Mfcc(80, 80) on the kernel's own log-mel; 1.31 on 2 x the grid's rows).
#
# K_SOFTMAX: softmax_rows_kernel (forward_softmax) and softmax_topk_kernel against oracle/topk_oracle.py::softmax_f64, per class in
# the unit of softmax_units
#     u = |got - p| / (eps p (1 + (m - l_i))),   eps = 2^-24, p the float64 posterior, m the row's maximum, l_i the class's logit
# (relative to the posterior ITSELF -- the absolute bars, 1e-6 / 1e-4 / 2^-15, pass an all-zero tail and 8 % in every class of a
# 2599-class row, whose typical posterior is 4e-4 -- plus the relative error (m - l_i) eps that one rounding of the exponent's
# argument leaves in exp).  Classes first: finite / the exact zero of a masked (-Inf) class / NaN at the oracle's positions, or the
# figure is infinite; a posterior below 2^-126 needs 0 <= got <= 2^-125 instead (at most 1 / 8 of a `deep/...` row, none elsewhere:
# tests/test_softmax_matrix.py asserts it from the oracle alone).  The rule of K_FBANK: the smallest power of two at or above TWICE
# the largest u of a plain float32 evaluation; the factor 2 is for the kernels' different but legitimate float32 order (per-lane
# online rescaling, a 64-lane butterfly, the hardware exponential on a base-2 argument).
# tests/test_softmax_matrix.py::test_k_softmax_is_twice_the_float32_evaluations asserts it.
#   * CPU, every row of tests/softmax_matrix.py (389 rows, 2.7 M logits: K = 1 .. 10007, eleven finite laws, seven mask placements,
#     NaN / +Inf rows):
#       numpy float32 two-pass (pairwise sum)                  4.67  (gauss3/K256)
#       ATen torch.softmax, float32                            9.26  (descending/K10007; with AVX512 kernels -- 13.9 with
#                                                              ATEN_CPU_CAPABILITY=avx2 or default: the same power of two) -> 32
#       the kernels' order, correctly rounded exp              5.35  (tests/softmax_matrix.py::kernel_order: inside K / 2, asserted)
#       strictly serial single-accumulator float32 sum         107   (gauss3/K10007): a CORRECT evaluation that the bar rejects, by
#                                                              design -- the bar separates summation orders.  Informational.
#     Both plain evaluations have the oracle's classes on every row.
#   * Negative controls, CPU emulations of the kernels' order with one defect (there is no device table to perturb), each on every
#     row of the matrix row named for it, CONTROL_MARGIN = 1.5 asked (48):
#       the K % 4 tail left out of the denominator             17,565 .. 19,804  (gauss0.1/K2599: 1.15e-3 relative; < 1e-6 absolute)
#       one lane's sum added without its rescale to the max    7.7e6 .. 8.2e6    (gauss12/K300)
#       the exponent's argument on a 2^-16 grid                118 .. 141        (gauss0.1/K2599)
#   * GPU (tests/test_hip_softmax_f64.py, every row through both kernels; per (kernel, law) in the error report of a GPU run under
#     softmax_f64/...):
#       softmax_rows_kernel   at most 4.14 (descending/K10007; gauss3 4.02, ascending 3.22, every mask placement <= 3.05, deep 2.05)
#       softmax_topk_kernel   at most 4.11 (descending/K10007; the same figures elsewhere: the worst class of a row is among its k best)
#       the five ties to forward(softmax = 1), bit-identical, on their models' own logits: <= 2.71
#     The hardware exponential on the rounded base-2 argument adds nothing the bar can see: the kernels sit BELOW the emulation
#     of their order with a correctly rounded exp (5.35 on the CPU) and 7.7 x below the bar.  The factor the rule leaves is ATen's
#     summation, not the kernels'.  tests/test_hip_topk.py under the added bar: its goldens, the 33,792-row call, 75 random shapes.
#     NOT measured: the negative controls on the device (the kernels have no table to perturb; CPU emulations alone).
#     The masked rows on the library BEFORE the guard (v == -Inf adds 0), softmax_topk through the C ABI, run once: 71 of the 95
#     masked rows (mask_all left out) came back with NaN probabilities, 31 with other indices than the oracle's (masked classes
#     were never ranked: -1).  softmax_rows_kernel of that library was not run on them: it has no entry point for chosen logits.
CONTROL_MARGIN = 1.5
K_FBANK = 16.0
K_DCT = 8.0
K_SOFTMAX = 32.0


def pow2_at_or_above(v):
    return 2.0 ** int(np.ceil(np.log2(v)))


POSTERIOR_TOL = 1e-4


def tol_for(ref):
    return POSTERIOR_TOL * max(1.0, float(np.abs(ref).max()))
