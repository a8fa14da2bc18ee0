#!/usr/bin/env python3
"""Generate tests/golden/criterion_golden.npz from the live reference: what wekws.model.loss.criterion returns for every
case of tests/criterion_matrix.py, plus -- for max_pooling -- the per-utterance correctness (the same function on one
utterance at a time) and the pooled values (its pooling statements, loss.py:55-70, run value by value: the function returns
only their sum), and -- for the accuracy -- the per-utterance edit distances from the reference's own
ctc_prefix_beam_search + Calculator.

It also measures what the bars of tests/criterion_matrix.py are derived from: the worst error of the reference's float32
results against the float64 oracle (tests/criterion_ref.py), in the unit documented there.
Build container only (needs /root/reference).

    python tests/golden/make_criterion_golden.py        (from the repository root)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, "/root/reference")
from wekws.model import loss as ref_loss  # noqa: E402

from tests import criterion_matrix as cm  # noqa: E402
from tests import criterion_ref as cr  # noqa: E402


def store_inputs(out, name, case, big):
    for k, v in case.items():
        v = np.asarray(v)
        if k == big and v.size > cm.SMALL:
            out[f"{name}/in/{k}_sum"] = np.float64(np.nansum(v.astype(np.float64)))
        else:
            out[f"{name}/in/{k}"] = v


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    out, worst = {}, {"max_pooling": 0.0, "ce": 0.0, "ctc": 0.0}

    for name in cm.case_names("max_pooling"):
        c = cm.max_pooling_case(name)
        s, tg, ln = torch.from_numpy(c["scores"]), torch.from_numpy(c["target"]), torch.from_numpy(c["lengths"])
        assert int(ln.max()) == s.size(1), name
        loss, acc = ref_loss.criterion("max_pooling", s, tg, ln, min_duration=c["min_duration"])
        B, T, K = s.shape
        pooled = np.empty((B, K), np.float32)
        terms = np.empty((B, K), np.float32)
        correct = np.zeros(B, np.int32)
        full = torch.tensor([T])
        for b in range(B):
            # per-utterance correctness from the live function: the utterance beside a full-length dummy (all zeros, target
            # K + 1: never correct), which keeps padding_mask at T columns; acc is then correct[b] / 2
            sb = torch.stack([s[b], torch.zeros(T, K)])
            _, a = ref_loss.max_pooling_loss(sb, torch.stack([tg[b], torch.tensor(K + 1, dtype=tg.dtype)]),
                                             torch.cat([ln[b:b + 1], full.to(ln.dtype)]), c["min_duration"])
            correct[b] = int(round(a * 2))
        # the function returns no pooled values: its own statements (loss.py:55-70), value by value, with torch's float32 ops
        mask = ref_loss.padding_mask(ln)
        for b in range(B):
            for j in range(K):
                if int(tg[b]) == j:
                    m = mask[b].clone()
                    m[:c["min_duration"]] = True
                    v = torch.clamp(s[b, :, j].masked_fill(m, 0.0), 1e-8, 1.0).max()
                else:
                    v = torch.clamp((1 - s[b, :, j]).masked_fill(mask[b], 1.0), 1e-8, 1.0).min()
                pooled[b, j] = v.item()
                terms[b, j] = (-torch.log(v)).item()
        o = cr.max_pooling(c["scores"], c["target"], c["lengths"], c["min_duration"])
        assert np.array_equal(pooled, o["pooled"], equal_nan=True), name
        assert np.array_equal(correct, o["correct"]), (name, correct, o["correct"])
        assert acc == o["acc"], (name, acc, o["acc"])
        u = max(cm.units(terms, o["terms"]), cm.units(np.float32(loss), o["loss"]))
        worst["max_pooling"] = max(worst["max_pooling"], u)
        store_inputs(out, name, c, "scores")
        out[name + "/loss"] = np.float32(loss)
        out[name + "/acc"] = np.float64(acc)
        out[name + "/pooled"] = pooled
        out[name + "/correct"] = correct
        print(f"{name:18s} loss {float(loss):.6f} acc {acc:.4f} ref units {u:.2f}")

    for name in cm.case_names("ce"):
        c = cm.ce_case(name)
        x, tg = torch.from_numpy(c["logits"]), torch.from_numpy(c["target"])
        loss, acc = ref_loss.criterion("ce", x, tg, None)
        rows = F.cross_entropy(x, tg.long(), reduction="none").numpy()
        pred = x.max(1)[1].numpy().astype(np.int32)
        o = cr.cross_entropy(c["logits"], c["target"])
        assert np.array_equal(pred, o["pred"]) and acc == o["acc"], name
        u = max(cm.units(rows, o["rows"]), cm.units(np.float32(loss), o["loss"]))
        worst["ce"] = max(worst["ce"], u)
        store_inputs(out, name, c, "logits")
        out[name + "/loss"] = np.float32(loss)
        out[name + "/acc"] = np.float64(acc)
        out[name + "/pred"] = pred
        print(f"{name:18s} loss {float(loss):.6f} acc {acc:.4f} ref units {u:.2f}")

    for name in cm.case_names("ctc"):
        c = cm.ctc_case(name)
        x, tg = torch.from_numpy(c["logits"]), torch.from_numpy(c["targets"]).long()
        ln, tl = torch.from_numpy(c["lengths"]).long(), torch.from_numpy(c["target_lengths"]).long()
        loss, acc = ref_loss.criterion("ctc", x, tg, ln, target_lengths=tl, validation=False)
        rows = F.ctc_loss(x.transpose(0, 1).log_softmax(2), tg, ln, tl, reduction="none").numpy()
        o = cr.ctc(c["logits"], c["targets"], c["lengths"], c["target_lengths"])
        u = max(cm.units(rows, o["rows"]), cm.units(np.float32(loss), o["loss"]))
        worst["ctc"] = max(worst["ctc"], u)
        store_inputs(out, name, c, "logits")
        out[name + "/loss"] = np.float32(loss)
        out[name + "/rows"] = rows.astype(np.float32)
        print(f"{name:18s} loss {float(loss):.6f} rows {np.array2string(rows, precision=3)} ref units {u:.2f}")

    for name in cm.case_names("acc"):
        c = cm.acc_case(name)
        x, tg = torch.from_numpy(c["logits"]), torch.from_numpy(c["targets"]).long()
        ln, tl = torch.from_numpy(c["lengths"]).long(), torch.from_numpy(c["target_lengths"]).long()
        loss, acc = ref_loss.criterion("ctc", x, tg, ln, target_lengths=tl, validation=True)
        probs = x.softmax(2)
        dist = np.zeros(len(ln), np.int32)
        words = errors = 0
        for b in range(len(ln)):
            hyps = ref_loss.ctc_prefix_beam_search(probs[b][:ln[b]], ln[b], None, 3, 5)
            r = ref_loss.Calculator().calculate([str(v) for v in tg[b][:tl[b]].tolist()], [str(v) for v in hyps[0][0]])
            dist[b] = r["ins"] + r["sub"] + r["del"]
            assert r["all"] == int(tl[b])
            words += r["all"]
            errors += int(dist[b]) if r["all"] else 0
            # the margins the case promises: every posterior is above 0.2 or below 1e-3
            pb = probs[b][:ln[b]].numpy()
            assert not ((pb > 1e-3) & (pb < 0.2)).any(), (name, b)
        assert acc == float(words - errors) * 100.0 / words
        # the result does not move when the posteriors are perturbed by 1e-6
        g = torch.Generator().manual_seed(1)
        for _ in range(3):
            xp = torch.log(probs + (torch.rand(probs.shape, generator=g) * 2 - 1) * 1e-6)
            _, acc2 = ref_loss.criterion("ctc", xp, tg, ln, target_lengths=tl, validation=True)
            assert acc2 == acc, (acc, acc2)
        o = cr.utterance_accuracy(c["logits"], c["targets"], c["lengths"], c["target_lengths"])
        assert np.array_equal(o["dist"], dist) and o["acc"] == acc, (o, dist, acc)
        o2 = cr.ctc(c["logits"], c["targets"], c["lengths"], c["target_lengths"])
        worst["ctc"] = max(worst["ctc"], cm.units(np.float32(loss), o2["loss"]))
        store_inputs(out, name, c, "logits")
        out[name + "/loss"] = np.float32(loss)
        out[name + "/acc"] = np.float64(acc)
        out[name + "/dist"] = dist
        out[name + "/totals"] = np.array([words, errors], np.int32)
        print(f"{name:18s} loss {float(loss):.6f} acc {acc:.4f} dist {dist.tolist()}")

    for k, v in worst.items():
        out[k + "/ref_units"] = np.float64(v)
        print(f"{k}: reference's worst error {v:.3f} units -> bar {2.0 ** int(np.ceil(np.log2(4 * v)))}")
    path = os.path.join(HERE, "criterion_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
