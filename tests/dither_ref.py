"""The yardstick of the dithered front end (CPU, numpy): Philox4x32-10 in integer arithmetic, the uniforms and the Box-Muller
transform in float64, the mapping from a frame's sample index to (Philox block, word), and the dithered frames themselves.

What the reference computes (torchaudio.compliance.kaldi._get_window, runtime/core/frontend/fbank.h:150-153): after the signal is
cut into frames and before DC removal, pre-emphasis and the window,  frame[i] += dither * N(0, 1)  -- an independent draw for every
(frame, sample), the signal in int16 scale.  The reference draws from torch's global CPU generator; that stream is not the contract.
The contract here (restated from wekws_amd/csrc/philox.hip.h, which states it once for the kernels):

  * generator  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123)
  * key        (seed & 0xffffffff, seed >> 32)
  * counter    (block within the frame, frame index, row id & 0xffffffff, row id >> 32)
  * mapping    sample i of a frame belongs to the sample pair n = i >> 1; pair n is served by
                   block  c0 = (n & 63) | ((n >> 7) << 6)          (the fbank lane l = n & 63 holds pairs l + 64 m, m = 0 .. 3:
                   words  w = 2 ((n >> 6) & 1),  w + 1              block l + 64 j serves its pairs m = 2 j and m = 2 j + 1)
  * uniforms   u = (2 (word >> 9) + 1) 2^-24: an odd multiple of 2^-24 in (0, 1), 24 significant bits -- exact in float32
               (u1 from word w, u2 from word w + 1).  ((word >> 8) + 0.5) 2^-24 would need 25 bits above 1/2.)  min u = 2^-24:
               |z| reaches sqrt(48 ln 2) = 5.77.
  * normals    r = sqrt(-2 ln u1);  the even sample 2 n gets r cos(2 pi u2), the odd sample 2 n + 1 gets r sin(2 pi u2)
  * addition   frame[i] = float32(x[i] + dither * z[i])  -- one rounding (the kernel: one fused multiply-add); samples past
               frame_length stay zero.

The frame oracle reuses oracle/fbank_oracle.py unchanged: the frames of a row, concatenated, are an utterance whose frame shift is
its frame length, so fbank_f64 / fbank_units evaluate each dithered frame on its own."""
import numpy as np

from oracle import fbank_oracle

M0, M1 = 0xD2511F53, 0xCD9E8D57                  # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                  # Weyl key increments
MASK = np.uint64(0xFFFFFFFF)

SEED = 0x5EEDD17E                                # the suite's seed
SEED_HI = (0xA5 << 32) | 0x00C0FFEE              # one above 2^32: the key's high word


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars -> four uint32 arrays."""
    c = [np.asarray(v, np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = c[0] * np.uint64(M0)
        p1 = c[2] * np.uint64(M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def uniform(word):
    """(2 (word >> 9) + 1) 2^-24 in float64 (exact there and in float32)."""
    return (2.0 * (np.asarray(word, np.uint32) >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24


def sample_map(i):
    """(block within the frame, first word) of sample i; the sample's normal is the cosine branch if i is even, else the sine."""
    n = np.asarray(i) >> 1
    return (n & 63) | ((n >> 7) << 6), 2 * ((n >> 6) & 1)


def _uniform_pairs(seed, first_row, B, nframes, frame_length):
    """(u1, u2) float64 arrays (B, nframes, frame_length) of the samples' pairs."""
    seed, first_row = int(seed), int(first_row)
    blk, w = sample_map(np.arange(frame_length))
    nblk = int(blk.max()) + 1
    rows = [first_row + b for b in range(B)]
    c2 = np.array([r & 0xFFFFFFFF for r in rows], np.uint64)[:, None, None]
    c3 = np.array([(r >> 32) & 0xFFFFFFFF for r in rows], np.uint64)[:, None, None]
    c1 = np.arange(nframes, dtype=np.uint64)[None, :, None]
    c0 = np.arange(nblk, dtype=np.uint64)[None, None, :]
    words = np.stack(philox4x32_10((c0, c1, c2, c3), (seed & 0xFFFFFFFF, seed >> 32)), axis=-1)     # (B, nframes, nblk, 4)
    return uniform(words[:, :, blk, w]), uniform(words[:, :, blk, w + 1])


def normal_field(seed, first_row, B, nframes, frame_length):
    """The (B, nframes, frame_length) unit-variance field in float64: what wekws_hip_dither_noise writes."""
    u1, u2 = _uniform_pairs(seed, first_row, B, nframes, frame_length)
    r = np.sqrt(-2.0 * np.log(u1))
    th = 2.0 * np.pi * u2
    even = (np.arange(frame_length) & 1) == 0
    return np.where(even, r * np.cos(th), r * np.sin(th))


def normal_field_f32(seed, first_row, B, nframes, frame_length):
    """The same formulas evaluated in numpy float32 from the same (exact) uniforms: the calibration of K_NOISE_Z."""
    f32 = np.float32
    u1, u2 = (v.astype(f32) for v in _uniform_pairs(seed, first_row, B, nframes, frame_length))
    r = np.sqrt(f32(-2.0) * np.log(u1))
    th = f32(2.0 * np.pi) * u2
    even = (np.arange(frame_length) & 1) == 0
    z = np.where(even, r * np.cos(th), r * np.sin(th))
    assert z.dtype == np.float32
    return z


def noise_units(got, ref):
    """Error of a noise field against the float64 one, per element, in units of 2^-24 max(1, |z|)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    u = np.abs(got - ref) / (2.0 ** -24 * np.maximum(1.0, np.abs(ref)))
    return np.where(np.isfinite(u), u, np.inf)


def frames_of(wave, frame_length, frame_shift):
    """(nframes, frame_length) float64 frames of a wave (snip edges, fbank.h:141-142)."""
    wave = np.asarray(wave, np.float64)
    nf = fbank_oracle.num_frames(wave.size, frame_length, frame_shift)
    idx = np.arange(frame_length)[None, :] + frame_shift * np.arange(nf)[:, None]
    return wave[idx]


def dithered_frames(wave, seed, row, frame_length, frame_shift, dither, z=None):
    """float64 frames of `wave` with dither * N(0, 1) added per (frame, sample), row id `row`.  z: another (nframes, frame_length)
    field to add instead (the negative controls)."""
    x = frames_of(wave, frame_length, frame_shift)
    if z is None:
        z = normal_field(seed, row, 1, x.shape[0], frame_length)[0]
    return x + np.float64(np.float32(dither)) * z


def frame_cfg(num_bins, sample_rate, frame_length, window):
    """The oracle functions' trailing arguments for frames evaluated one by one: the shift is the frame length."""
    return num_bins, sample_rate, frame_length, frame_length, window


def frame_units(got, frames, num_bins, sample_rate, frame_length, window):
    """fbank_units of the features `got` (nframes, bins) of already cut `frames` (nframes, frame_length)."""
    return fbank_oracle.fbank_units(got, np.asarray(frames).reshape(-1), *frame_cfg(num_bins, sample_rate, frame_length, window))


# ---------------------------------------------------------------------------------------------------------------------
# The bars.  Both follow the rule of tests/helpers.py (K_FBANK): the smallest power of two at or above TWICE the largest figure of a
# plain float32 evaluation; tests/test_dither_ref.py asserts both from the measurements named here.
#
# K_NOISE_Z, the noise field in units of 2^-24 max(1, |z|): normal_field_f32 against normal_field over the GPU test's fields.  The
# float32 figure is dominated by the rounding of the angle 2 pi u2 (up to 2^-22 absolute at the top of the range) times r.
# The kernels (explicit range reduction, philox.hip.h) measure 3.91 at the most on the device, 0.6 rms.
K_NOISE_Z = 64.0          # float32 figure 21.71 over NOISE_FIELDS (31.28 over the 2^20 values of the distribution test: the same bar)
NOISE_FIELDS = [(3, 7, 400), (2, 5, 512), (2, 5, 65), (1, 3, 401)]                       # (B, nframes, frame_length)
NOISE_FIRST_ROWS = (0, 5, 2 ** 33 + 1)
# The features, in fbank_units against fbank_f64 of the dithered float64 frames (each frame a one-frame utterance):
#   * noise and silence rows: fbank_f32_exact on float32(x + float32(dither z)) reaches 5.43 over CASES (noise, b40_ham_i16_pair_d375;
#     silence 5.13): within K_FBANK / 2 = 8, so these rows are held to K_FBANK itself.
#   * the full-scale DC rows are another matter, on BOTH sides: the frame is 32767 + dither z, its float32 mean carries the rounding
#     of a sum of 1.3e7 (an error of the order of 2^-9 .. 2^-7 left in every sample) while fbank_units' noise scale S is taken on the
#     DC-removed frame, whose size is dither.  The float32 restatement reaches 47 (dither 37.5) .. 14789 (dither 0.25) there, the
#     figure growing as 1 / dither.  The issue's rule -- the smallest power of two at or above twice the float32 figure -- is applied
#     per case, so that a row with a large dither is not handed the bar of one with a small dither: K_DITHER_DC, the measured float32
#     figure beside each.  test_dither_ref.py::test_bars_follow_the_float32_restatement asserts every entry.
K_DITHER_DC = {
    "b40_ham_f32_pair_d1": 4096.0,             # 1356.74
    "b80_pov_f32_pair_d1": 16384.0,            # 6967.76
    "b40_ham_i16_pair_d1": 4096.0,             # 1356.74
    "b80_pov_i16_single_d1": 16384.0,          # 6967.76
    "b40_ham_f32_single_d025": 16384.0,        # 7619.54
    "b80_pov_f32_pair_d375": 512.0,            # 158.06
    "b40_ham_i16_pair_d375": 128.0,            # 47.45
    "b40_ham_f32_f512_pair_d1": 2048.0,        # 893.36
    "b80_pov_f32_f512_single_d025": 32768.0,   # 14789.37
    "b23_ham_f32_f65_d1": 16384.0,             # 4949.00
    "b23_pov_i16_f65_d375": 512.0,             # 147.64
    "b40_ham_i16_noshift_single_d025": 8192.0,  # 3852.81
    "b80_pov_i16_noshift_pair_d1": 16384.0,    # 6967.76
}


def case_bar(case, kind):
    """The bar of a row of a case, in fbank_units: K_FBANK, or the DC row's own (above)."""
    from tests.helpers import K_FBANK
    return K_DITHER_DC[case["id"]] if kind == "dc" else K_FBANK


def f32_restatement(case, b):
    """(features of fbank_f32_exact on float32(x + float32(dither z)), the float64 dithered frames) of row b of a case."""
    x = case_input(case)[b]
    nf = fbank_oracle.num_frames(case["nsamp"], case["flen"], case["shift"])
    z = normal_field(SEED, FIRST_ROW + b, 1, nf, case["flen"])[0]
    frames = dithered_frames(x, SEED, FIRST_ROW + b, case["flen"], case["shift"], case["dither"], z=z)
    noise = (np.float32(case["dither"]) * z.astype(np.float32)).astype(np.float32)
    f32 = (frames_of(x, case["flen"], case["shift"]).astype(np.float32) + noise).astype(np.float32)
    return fbank_oracle.fbank_f32_exact(f32.reshape(-1), *frame_cfg(*case_cfg(case))), frames

# ---------------------------------------------------------------------------------------------------------------------
# The cases of the feature test (tests/test_hip_dither.py) and of the bar's calibration (tests/test_dither_ref.py).  Every case is
# B = 3 rows -- noise, silence, a full-scale DC offset (32767 in every sample) -- integer valued, so the int16 cases carry the same
# samples.  23 bins at frames of 65 samples: the most that framing carries without an empty filter (tests/fbank_matrix.py).
def _case(cid, bins, window, dtype, nsamp, flen, shift, dither):
    return dict(id=cid, bins=bins, window=window, dtype=dtype, nsamp=nsamp, flen=flen, shift=shift, dither=dither, sr=16000, B=3)


CASES = [
    _case("b40_ham_f32_pair_d1", 40, 0, "f32", 16000, 400, 160, 1.0),
    _case("b80_pov_f32_pair_d1", 80, 1, "f32", 16000, 400, 160, 1.0),
    _case("b40_ham_i16_pair_d1", 40, 0, "i16", 16000, 400, 160, 1.0),
    _case("b80_pov_i16_single_d1", 80, 1, "i16", 15999, 400, 160, 1.0),
    _case("b40_ham_f32_single_d025", 40, 0, "f32", 15999, 400, 160, 0.25),
    _case("b80_pov_f32_pair_d375", 80, 1, "f32", 16000, 400, 160, 37.5),
    _case("b40_ham_i16_pair_d375", 40, 0, "i16", 16000, 400, 160, 37.5),
    _case("b40_ham_f32_f512_pair_d1", 40, 0, "f32", 16000, 512, 160, 1.0),
    _case("b80_pov_f32_f512_single_d025", 80, 1, "f32", 15999, 512, 160, 0.25),
    _case("b23_ham_f32_f65_d1", 23, 0, "f32", 4000, 65, 33, 1.0),
    _case("b23_pov_i16_f65_d375", 23, 1, "i16", 4000, 65, 33, 37.5),
    _case("b40_ham_i16_noshift_single_d025", 40, 0, "i16", 15999, 400, 400, 0.25),
    _case("b80_pov_i16_noshift_pair_d1", 80, 1, "i16", 16000, 400, 400, 1.0),
]
KINDS = ("noise", "silence", "dc")
FIRST_ROW = 5                                     # the cases' first row id (row b: FIRST_ROW + b)


def case_input(case):
    """(3, nsamp) float32 in int16 scale, integer valued: noise, silence, the full-scale DC offset."""
    from wekws_amd.utils import synth
    x = np.zeros((3, case["nsamp"]), np.float32)
    x[0] = synth.synth_pcm(1, case["nsamp"], seed=31, kind="noise")[0]
    x[2] = 32767.0
    return x


def case_cfg(case):
    return case["bins"], case["sr"], case["flen"], case["window"]
