"""Runs every row of tests/fbank_matrix.py on the GPU with the TEST build of the library (libwekws_hip_hooks.so: the launch record
wekws_hip_debug_fbank_last, the table hook wekws_hip_debug_fbank_tables), for tests/test_hip_fbank_f64.py.  Run as a subprocess
with WEKWS_HIP_LIB pointing at it:

    python tests/tools/fbank_matrix_cases.py OUT.jsonl [row ids]

Per row: the variant the launch ran (rounds, sample size, pair_ok and grid as launch_fbank recorded them; stride and the widest
filter are properties of the table, taken from the table plan of the same configuration), the grid against one resident round, the
mel weights of the handle's device table against the oracle's bank bit for bit; every bin of every frame of every utterance in
fbank_units against the float64 oracle; the other sample type bit for bit.  The large-batch rows compare a fixed sample of
utterances with the oracle and EVERY utterance, bit for bit, with the same utterances run in batches of 8.  Rows named for the
negative controls run again on a perturbed device table (restored and re-checked afterwards).  One JSON record per row; nothing is
run again after a failure: the first exception ends the process."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import fbank_oracle  # noqa: E402
from tests import fbank_matrix as fm  # noqa: E402
from wekws_amd import _capi  # noqa: E402
from wekws_amd.frontend import Fbank  # noqa: E402


def device_input(x, dtype, off):
    """x (B, n) on the device as float32 or int16, starting `off` samples into its allocation."""
    t = torch.from_numpy(x if dtype == "f32" else x.astype(np.int16))
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (off * t.element_size()) % 16
    return v


def read_table(lib, fb, n):
    t = np.empty(n, np.float32)
    _capi.check(lib.wekws_hip_debug_fbank_tables(fb._ptr, t.ctypes.data, n, 0), "wekws_hip_debug_fbank_tables")
    return t


def write_table(lib, fb, t):
    t = np.ascontiguousarray(t, np.float32)
    _capi.check(lib.wekws_hip_debug_fbank_tables(fb._ptr, t.ctypes.data, t.size, 1), "wekws_hip_debug_fbank_tables")


def control_table(name, row, p, t):
    """The perturbed copy of device table t (layout: fbank.hip.h::FbankParams) and the mel bin the control touches (or -1)."""
    t = t.copy()
    ns, bins = p["nslots"], row["bins"]
    sbin = t[p["slot_bin_off"]:p["slot_bin_off"] + ns].astype(int)
    sfirst = t[p["slot_first_off"]:p["slot_first_off"] + ns].astype(int)
    sw = t[p["slot_w_off"]:p["slot_w_off"] + 16 * ns].reshape(ns, 16)           # (a view: writes go to t)
    if name in ("twiddle", "coarse_twiddle"):                                    # both tables by the reference's float32 recurrence / on a 2^-18 grid
        make = fbank_oracle.TWIDDLES["recurrence" if name == "twiddle" else "coarse"]
        t[0:512] = make(256, 256).ravel()
        t[512:1024] = make(512, 256).ravel()
        return t, -1
    if name == "weight":                                                         # the centre weight of the middle filter x (1 + 2^-12)
        b = bins // 2
        s = np.flatnonzero(sbin == b)
        k = np.unravel_index(int(np.argmax(sw[s])), (s.size, 16))
        sw[s[k[0]], k[1]] *= np.float32(1.0 + 2.0 ** -12)
        return t, b
    if name == "mel_double":                                                     # the bank computed in double, then rounded
        W = fbank_oracle.mel_bank(bins, row["sr"], row["flen"], double=True)
        for s in range(ns):
            for u in range(16):
                k = sfirst[s] + u
                inside = sw[s, u] != 0.0
                if inside:
                    assert k % p["stride"] == 0
                    sw[s, u] = W[sbin[s], k // p["stride"]]
        return t, -1
    raise ValueError(name)


def bank_equal(row, p, t):
    """Are the slot weights of device table t the oracle's mel bank (fbank_oracle.mel_bank), bit for bit, every tap of every slot at
    its place in the 512-point spectrum and zeros between the reference's bins?"""
    ns = p["nslots"]
    sbin = t[p["slot_bin_off"]:p["slot_bin_off"] + ns].astype(int)
    sfirst = t[p["slot_first_off"]:p["slot_first_off"] + ns].astype(int)
    sw = t[p["slot_w_off"]:p["slot_w_off"] + 16 * ns].reshape(ns, 16)
    W = fbank_oracle.mel_bank(row["bins"], row["sr"], row["flen"])
    full = np.zeros((row["bins"], 256 + 16), np.float32)
    full[:, 0:256:p["stride"]] = W
    have = np.zeros_like(full)
    for s in range(ns):
        have[sbin[s], sfirst[s]:sfirst[s] + 16] += sw[s]
    return bool(np.array_equal(have.view(np.int32), full.view(np.int32)))


def run_row(lib, row):
    cfg = fm.row_cfg(row)
    p = fm.plan(lib, *cfg)
    fb = Fbank(num_bins=row["bins"], sample_rate=row["sr"], frame_length=row["flen"], frame_shift=row["shift"], window=row["window"])
    other = "i16" if row["dtype"] == "f32" else "f32"
    B = row["B"]
    if row["grid"]:                                            # the resident round of this (kernel, device, sample type): one small launch
        fb(device_input(fm.row_input(row, 1), row["dtype"], 0))
        B = fm.large_batch(row, fm.last(lib)["resident"], p["fw"], p["waves"])
    x = fm.row_input(row, B)
    got_t = fb(device_input(x, row["dtype"], row["x_off"]))
    torch.cuda.synchronize()
    tr = fm.last(lib)
    got = got_t.cpu().numpy()
    rec = dict(id=row["id"], B=B, grid=tr["grid"], resident=tr["resident"], launch=[tr["B"], tr["nsamp"], tr["nframes"]],
               wanted_groups=-(-B * row["nframes"] // (p["fw"] * p["waves"])),
               variant=fm.variant_str(tr["rounds"], p["stride"], tr["pair_ok"], {4: "f32", 2: "i16"}[tr["sample_bytes"]], p["widest"]))
    assert got.shape == (B, row["nframes"], row["bins"]), got.shape
    # the other sample type, bit for bit (an aligned buffer: the comparison is of the arithmetic, not of the load path)
    alt = fb(device_input(x, other, 0))
    rec["other_type_equal"] = bool(torch.equal(alt.view(torch.int32), got_t.view(torch.int32)))
    which = list(range(B))
    if row["grid"]:
        which = fm.sample_utterances(B, row["nframes"], tr["grid"], p["fw"], p["waves"])
        small = torch.cat([fb(device_input(x[i:i + 8], row["dtype"], row["x_off"])) for i in range(0, B, 8)])
        rec["batches_of_8_equal"] = bool(torch.equal(small.view(torch.int32), got_t.view(torch.int32)))
    u = fm.units(row, got[which], x[which])
    rec["checked"] = len(which)
    rec["u"] = float(u.max())
    rec["u_kind"] = {k: float(u[[j for j, i in enumerate(which) if i % 4 == n]].max(initial=0.0)) for n, k in enumerate(fm.KINDS)}
    j, f, b = np.unravel_index(int(u.argmax()), u.shape)
    rec["worst"] = [int(which[j]), int(f), int(b)]
    rec["controls"] = {}
    table = read_table(lib, fb, p["table_floats"])
    rec["bank_equal"] = bank_equal(row, p, table)
    if row["controls"]:
        for name in row["controls"]:
            pert, b = control_table(name, row, p, table)
            write_table(lib, fb, pert)
            cu = fm.units(row, fb(device_input(x, row["dtype"], row["x_off"])).cpu().numpy(), x)
            write_table(lib, fb, table)
            per_bin = cu.max(axis=(0, 1))
            rec["controls"][name] = dict(u=float(cu.max()), bin=b, u_bin=float(per_bin[b]) if b >= 0 else None,
                                         u_other=float(np.delete(per_bin, b).max()) if b >= 0 else None)
        back = fb(device_input(x, row["dtype"], row["x_off"]))
        rec["restored"] = bool(torch.equal(back.view(torch.int32), got_t.view(torch.int32)))
    return rec


def main():
    out = sys.argv[1]
    lib = fm.type_hooks(_capi.load())
    assert _capi.lib_path().endswith("libwekws_hip_hooks.so"), _capi.lib_path()
    only = sys.argv[2:]
    with open(out, "w") as f:
        for row in fm.ROWS:
            if only and row["id"] not in only:
                continue
            f.write(json.dumps(run_row(lib, row)) + "\n")
            f.flush()
    print("OK")


if __name__ == "__main__":
    main()
