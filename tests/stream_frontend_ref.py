"""Host restatement of the streaming front end (KeyWordSpotter.accept_wave, wekws/bin/stream_kws_ctc.py:335-398) in INDEX
space: which global fbank frame of a stream lands in which slot of which output row.  Frame k of a stream is samples
[k S, k S + L) of its whole signal, so a row of the front end is fully described by the global frames of its
left + right + 1 slots.  Pinned against the live reference by tests/golden/stream_frontend_golden.npz
(make_stream_frontend_golden.py); tests gather one-shot features with these indices to get the expected rows."""
from __future__ import annotations

from typing import List, Optional

import numpy as np

HELD = "held"        # the reference's None
ASSERT = "assert"    # the reference's `assert feat_len > self.right_context`


class StreamRef:
    """One stream.  ``push(n)`` returns HELD, ASSERT (no state change, as the library refuses the call) or an int array
    (rows, left + right + 1) of global frame indices; ``counts()`` is (rem, fr or -1, off)."""

    def __init__(self, L: int, S: int, left: int = 0, right: int = 0, skip: int = 1):
        self.L, self.S, self.l, self.r, self.ds = L, S, left, right, skip
        self.ctx = left > 0 or right > 0
        self.reset()

    def reset(self):
        self.rem = 0
        self.fr: Optional[List[int]] = None
        self.off = 0
        self.base = 0          # global index of the first sample still held: S times the frames produced so far
        self.rows_total = 0

    def counts(self):
        return self.rem, (-1 if self.fr is None else len(self.fr)), self.off

    def push(self, n: int):
        L, S, l, r, ds = self.L, self.S, self.l, self.r, self.ds
        tot = self.rem + n
        if tot < L * r:                                   # 1. hold
            self.rem = tot
            return HELD
        nf = 0 if tot < L else 1 + (tot - L) // S         # 2. fbank over [rem | chunk]
        assert self.base % S == 0
        k0 = self.base // S
        new = list(range(k0, k0 + nf))
        if self.ctx and not nf > r:                       # 3. the reference's assertion
            return ASSERT
        self.rem = tot - nf * S
        self.base += nf * S
        W = l + r + 1
        if self.ctx:
            pad = [new[0]] * l + new if self.fr is None else self.fr + new
            rows = [pad[i:i + W] for i in range(max(len(pad) - 2 * r, 0))]
            self.fr = new[-(l + r):]
        else:
            rows = [[k] for k in new]
        if ds > 1:                                        # 4. skip
            k = len(rows)
            rows = rows[self.off::ds]
            self.off = (self.off - k) % ds
        self.rows_total += len(rows)
        return np.asarray(rows, dtype=np.int64).reshape(len(rows), W)


def run_schedule(L, S, left, right, skip, sizes):
    """[(result, counts after)] of one stream fed `sizes`; stops after an ASSERT."""
    s = StreamRef(L, S, left, right, skip)
    out = []
    for n in sizes:
        res = s.push(int(n))
        out.append((res, s.counts()))
        if isinstance(res, str) and res == ASSERT:
            break
    return out


def is_marker(res, what) -> bool:
    return isinstance(res, str) and res == what
