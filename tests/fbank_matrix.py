"""The fbank kernel's variant matrix: rows that each NAME the variant of fbank_kernel they run -- mel slots per lane (ROUNDS),
spectrum stride (512 / the reference's transform length), the paired or the per-sample loads, the sample type, the widest filter's
slot count, the persistent grid -- the way tests/route_matrix.py names conv routes.  Shared by
  * tests/test_fbank_matrix.py (CPU): every row's name equals wekws_hip_debug_fbank_plan (fbank_build_tables run without a device),
    a sweep of the configuration space finds the reachable (rounds, stride, pair_ok, sample type) tuples and none lacks a row, the
    float32 calibration of the bar and the CPU emulation of the negative controls;
  * tests/tools/fbank_matrix_cases.py -> tests/test_hip_fbank_f64.py (GPU): every row on the device with the hooks library, the
    launch record against the name, every bin against the float64 oracle in fbank_units at K_FBANK.
An utterance of a row is one of four inputs by its index: noise, a sine, the int16 full-range ramp, silence."""
import ctypes as C
import os

import numpy as np

from wekws_amd import _capi
from wekws_amd.utils import synth

KINDS = ("noise", "sine", "ramp", "silence")
WINDOWS = ("hamming", "povey")
PLAN_KEYS = ("rounds", "nslots", "stride", "widest", "fw", "waves", "mel_first_off", "mel_size_off", "mel_start_off", "mel_w_off",
             "mel_w_count", "slot_first_off", "slot_bin_off", "slot_w_off", "table_floats", "empty")
LAST_KEYS = ("rounds", "sample_bytes", "pair_ok", "grid", "resident", "B", "nsamp", "nframes")


def hooks_path():
    return os.path.join(os.path.dirname(_capi.lib_path()), "libwekws_hip_hooks.so")


def type_hooks(lib):
    lib.wekws_hip_debug_fbank_plan.restype = C.c_int
    lib.wekws_hip_debug_fbank_plan.argtypes = [C.POINTER(_capi.FbankCfg), C.POINTER(C.c_int)]
    lib.wekws_hip_debug_fbank_last.restype = C.c_int
    lib.wekws_hip_debug_fbank_last.argtypes = [C.POINTER(C.c_int)]
    lib.wekws_hip_debug_fbank_tables.restype = C.c_int
    lib.wekws_hip_debug_fbank_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return lib


def plan(lib, bins, sr, flen, shift=160, window=0):
    """wekws_hip_debug_fbank_plan as a dict (PLAN_KEYS); empty >= 0: that filter covers no FFT bin, the configuration is refused."""
    cfg = _capi.FbankCfg()
    cfg.num_bins, cfg.sample_rate, cfg.frame_length, cfg.frame_shift, cfg.window = bins, sr, flen, shift, window
    out = (C.c_int * 16)()
    rc = lib.wekws_hip_debug_fbank_plan(C.byref(cfg), out)
    assert rc == 0, (rc, bins, sr, flen)
    return dict(zip(PLAN_KEYS, out))


def last(lib):
    out = (C.c_int * 8)()
    assert lib.wekws_hip_debug_fbank_last(out) == 0
    return dict(zip(LAST_KEYS, out))


def pair_ok(nsamp, shift, flen, x_off, dtype):
    """The kernel's condition for its paired loads, for a buffer that starts x_off samples into an allocation aligned to 16 bytes."""
    size = 4 if dtype == "f32" else 2
    return int(nsamp % 2 == 0 and shift % 2 == 0 and flen % 2 == 0 and (x_off * size) % (2 * size) == 0)


def variant_str(rounds, stride, pair, dtype, widest):
    return f"rounds{rounds} stride{stride} {'pair' if pair else 'single'} {dtype} slots{widest}"


def _row(rid, variant, bins, sr, flen, shift, nframes, B, window="hamming", dtype="f32", extra=0, x_off=0, grid=None, controls=()):
    """nsamp = flen + (nframes - 1) shift + extra.  grid: None, or ("over" | "under", workgroups of the launch relative to one
    resident round) for the two large-batch rows (B is then set on the device from the handle's resident count).  controls: the
    negative controls this row is named for."""
    return dict(id=rid, variant=variant, bins=bins, sr=sr, flen=flen, shift=shift, nframes=nframes, B=B, window=window, dtype=dtype,
                nsamp=flen + (nframes - 1) * shift + extra, x_off=x_off, grid=grid, controls=tuple(controls))


# 16 kHz / 25 ms / 10 ms is the runtime's framing; 8 kHz (200 samples, 256 points) and 4 kHz (100 samples, 128 points) are its
# stride-2 and stride-4 cases.  A filter of n reference bins spans (n - 1) stride + 1 bins of the 512-point spectrum and is cut into
# slots of 16.  kFbankFW (frames per wave) is 1 in this build, so "kFbankFW +- 1 frames" are the 2-frame rows (0 frames launch nothing).
BASES = {  # (rounds, stride): (tag, sample rate, frame length, shift, bins, widest filter's slots)
    (1, 1): ("k16_b40", 16000, 400, 160, 40, 2), (2, 1): ("k16_b80", 16000, 400, 160, 80, 1),
    (1, 2): ("k8_b40", 8000, 200, 80, 40, 2), (2, 2): ("k8_b80", 8000, 200, 80, 80, 1),
    (1, 4): ("k4_b40", 4000, 100, 40, 40, 2), (2, 4): ("k4_b66", 4000, 100, 40, 66, 1),     # (66: the most bins 4 kHz / 128 points carry)
}
# The negative controls, each a perturbed device table (tests/tools/fbank_matrix_cases.py::control_table) with a CPU emulation
# (oracle/fbank_oracle.py::fbank_f32_exact): "weight", "mel_double" and "coarse_twiddle" must MISS the bar; "twiddle" (both tables
# by the reference's float32 recurrence) must stay INSIDE it -- see K_FBANK in tests/helpers.py for why.
CONTROLS = ("twiddle", "coarse_twiddle", "weight", "mel_double")
CONTROL_EMULATION = dict(twiddle=dict(fft="table", twiddles="recurrence"), coarse_twiddle=dict(fft="table", twiddles="coarse"),
                         mel_double=dict(mel="double"))                      # ("weight": weight=(bins // 2, 1 + 2^-12))
CONTROL_ROWS = ("k16_b80_pair_f32", "k16_b80_pov_pair_f32", "k8_b40_pair_f32")               # noise at 80 bins (both windows), 8 kHz noise

ROWS = []
for (_r, _s), (_tag, _sr, _fl, _sh, _b, _w) in sorted(BASES.items()):
    # every (rounds, stride) x paired / per-sample loads x float / int16; the per-sample path once by an odd sample count, once by an odd shift
    ROWS += [
        _row(f"{_tag}_pair_f32", variant_str(_r, _s, 1, "f32", _w), _b, _sr, _fl, _sh, 13, 4,
             controls=CONTROLS if f"{_tag}_pair_f32" in CONTROL_ROWS else ()),
        _row(f"{_tag}_pair_i16", variant_str(_r, _s, 1, "i16", _w), _b, _sr, _fl, _sh, 13, 4, window="povey", dtype="i16"),
        _row(f"{_tag}_oddn_f32", variant_str(_r, _s, 0, "f32", _w), _b, _sr, _fl, _sh, 13, 4, window="povey", extra=1),
        _row(f"{_tag}_oddshift_i16", variant_str(_r, _s, 0, "i16", _w), _b, _sr, _fl, _sh + 1, 13, 4, dtype="i16"),
    ]
ROWS += [
    _row("k16_b80_pov_pair_f32", "rounds2 stride1 pair f32 slots1", 80, 16000, 400, 160, 13, 4, window="povey",
         controls=CONTROLS),
    # ---- the pointer: aligned to one sample but not to a pair (a tensor sliced by one element)
    _row("k16_b40_off1_f32", "rounds1 stride1 single f32 slots2", 40, 16000, 400, 160, 13, 4, x_off=1),
    _row("k16_b80_off1_i16", "rounds2 stride1 single i16 slots1", 80, 16000, 400, 160, 13, 4, dtype="i16", x_off=1, window="povey"),
    _row("k16_b40_off2_f32", "rounds1 stride1 pair f32 slots2", 40, 16000, 400, 160, 13, 4, x_off=2),
    # ---- bin counts 23 / 64 (40 and 80 above), the most bins this framing carries (126; 127 leaves a filter empty), 128 bins
    _row("k16_b23", "rounds1 stride1 pair f32 slots4", 23, 16000, 400, 160, 13, 4),
    _row("k16_b64", "rounds2 stride1 pair f32 slots2", 64, 16000, 400, 160, 13, 4, window="povey"),
    _row("k16_b126", "rounds2 stride1 pair f32 slots1", 126, 16000, 400, 160, 13, 4),
    _row("k8_f400_b128", "rounds2 stride1 pair f32 slots1", 128, 8000, 400, 160, 13, 4, window="povey"),
    # ---- filters of 3 slots (1, 2 and 4 above), and ONE filter over the whole spectrum: 16 slots, one mel bin
    _row("k8_b23", "rounds1 stride2 pair f32 slots3", 23, 8000, 200, 80, 13, 4),
    _row("k4_b23", "rounds1 stride4 pair i16 slots3", 23, 4000, 100, 40, 13, 4, dtype="i16"),
    _row("k2_f300_b1", "rounds1 stride1 pair f32 slots16", 1, 2000, 300, 100, 13, 4),
    # ---- frame lengths at the edges of the three transform lengths: 65, 128 | 129, 256 | 257, 512 (400 above); odd ones load per sample
    _row("k16_f65", "rounds1 stride4 single f32 slots4", 23, 16000, 65, 32, 13, 4),
    _row("k16_f128", "rounds1 stride4 pair f32 slots4", 23, 16000, 128, 64, 13, 4, window="povey"),
    _row("k16_f129", "rounds1 stride2 single i16 slots4", 23, 16000, 129, 64, 13, 4, dtype="i16"),
    _row("k16_f256", "rounds1 stride2 pair f32 slots2", 40, 16000, 256, 128, 13, 4),
    _row("k16_f257", "rounds2 stride1 single f32 slots1", 80, 16000, 257, 128, 13, 4, window="povey"),
    _row("k16_f512", "rounds2 stride1 pair i16 slots1", 80, 16000, 512, 160, 13, 4, dtype="i16"),
    # ---- 1 and 2 frames per utterance, B > 1: a workgroup's four waves straddle utterances
    _row("k16_b40_nf1", "rounds1 stride1 pair f32 slots2", 40, 16000, 400, 160, 1, 7, extra=158),
    _row("k16_b80_nf2", "rounds2 stride1 pair i16 slots1", 80, 16000, 400, 160, 2, 7, dtype="i16", window="povey"),
    _row("k4_b40_nf1_odd", "rounds1 stride4 single f32 slots2", 40, 4000, 100, 40, 1, 5, extra=39),
    _row("k8_b80_nf2", "rounds2 stride2 pair f32 slots1", 80, 8000, 200, 80, 2, 5),
    # ---- the persistent grid: more workgroups than one resident round (every wave walks several strides and carries (utterance,
    #      frame) across them; 21 frames per utterance, so a stride ends inside an utterance), one frame per utterance, just under
    _row("k16_b80_over", "rounds2 stride1 pair f32 slots1", 80, 16000, 400, 160, 21, 0, grid=("over", 3.3)),
    _row("k16_b40_over_nf1", "rounds1 stride1 pair i16 slots2", 40, 16000, 400, 160, 1, 0, dtype="i16", grid=("over", 2.6)),
    _row("k8_b40_over_odd", "rounds1 stride2 single f32 slots2", 40, 8000, 200, 81, 21, 0, window="povey", grid=("over", 2.2)),
    _row("k16_b40_under", "rounds1 stride1 pair f32 slots2", 40, 16000, 400, 160, 21, 0, grid=("under", 1.0)),
]
assert len({r["id"] for r in ROWS}) == len(ROWS)


def row_cfg(row):
    """(num_bins, sample_rate, frame_length, frame_shift, window index): the oracle functions' trailing arguments."""
    return row["bins"], row["sr"], row["flen"], row["shift"], WINDOWS.index(row["window"])


def row_variant(lib, row):
    """The row's variant as fbank_build_tables and the kernel's own pair condition give it."""
    p = plan(lib, *row_cfg(row))
    assert p["empty"] < 0, (row["id"], p["empty"])
    return variant_str(p["rounds"], p["stride"], pair_ok(row["nsamp"], row["shift"], row["flen"], row["x_off"], row["dtype"]), row["dtype"],
                       p["widest"])


def variant_tuple(v):
    """(rounds, stride, pair_ok, sample type) of a variant string."""
    r, s, p, d, _ = v.split()
    return int(r[6:]), int(s[6:]), int(p == "pair"), d


def large_batch(row, resident, fw=1, waves=4):
    """B of a large-batch row on a device whose resident round is `resident` workgroups: `factor` strides of the capped grid ("over"),
    or the most utterances whose grid stays under one resident round ("under")."""
    kind, factor = row["grid"]
    per_group = fw * waves
    if kind == "over":
        return int(np.ceil(factor * resident * per_group / row["nframes"]))
    return ((resident - 1) * per_group) // row["nframes"]


def sample_utterances(B, nframes, grid, fw=1, waves=4):
    """The utterances of a large-batch row that are compared with the float64 oracle: first and last, those either side of every
    wrap of the wave stride (frames k stride - 1 and k stride), one in 97."""
    stride = grid * fw * waves
    s = {0, B - 1} | set(range(0, B, 97))
    for f in range(stride, B * nframes, stride):
        s |= {(f - 1) // nframes, f // nframes}
    return sorted(s)


def row_input(row, B=None):
    """(B, nsamp) float32 in int16 scale (integer-valued: the int16 rows carry the same samples): utterance i is KINDS[i % 4]."""
    B = row["B"] if B is None else B
    n = row["nsamp"]
    x = np.zeros((B, n), np.float32)
    for k, kind in enumerate(KINDS):
        idx = np.arange(k, B, 4)
        if idx.size and kind != "silence":
            part = synth.synth_pcm(idx.size, n, seed=17 + k, kind=kind)
            if kind == "sine":                                           # (synth's sine is the same for every utterance: another pitch each)
                t = np.arange(n, dtype=np.float64) / row["sr"]
                f0 = row["sr"] * (0.031 + 0.0173 * (np.arange(idx.size) % 23))[:, None]
                part = np.round(8000.0 * np.sin(2 * np.pi * f0 * t[None, :])).astype(np.float32)
            x[idx] = part
    return x


def units(row, got, x):
    """fbank_units of every utterance: (B, frames, bins)."""
    from oracle import fbank_oracle
    return np.stack([fbank_oracle.fbank_units(got[i], x[i], *row_cfg(row)) for i in range(x.shape[0])])


# ---- the DCT / lifter kernel (tests/test_hip_mfcc_f64.py, calibrated in tests/test_fbank_matrix.py): (rows, bins, cepstra, lifter) -- the
# four shapes of tests/test_kaldi_feats.py::test_hip_mfcc, one cepstrum, row counts around the kernel's 16-row tile, every square shape 1 .. 128
DCT_SHAPES = [(1, 80, 80, 22.0), (37, 80, 80, 22.0), (1000, 40, 13, 22.0), (50, 23, 23, 0.0), (5, 40, 1, 22.0)]
DCT_SHAPES += [(r, 80, 80, 22.0) for r in (15, 16, 17, 31, 32, 33)] + [(3, n, n, 22.0) for n in range(1, 129)]


def dct_input(rows, nb, seed=0):
    """Log-mel-like rows: values around 10 +- 5, every 7th element at the log floor."""
    x = (np.random.default_rng([seed, rows, nb]).standard_normal((rows, nb)) * 5 + 10).astype(np.float32)
    x.ravel()[::7] = np.float32(np.log(np.finfo(np.float32).eps))
    return x
