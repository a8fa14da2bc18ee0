#!/usr/bin/env python3
"""Global CMVN statistics of a wav.scp on the device: the reference's tools/compute_cmvn_stats.py with its arguments.

    python -m wekws_amd.bin.compute_cmvn_stats --train_config conf/ds_tcn.yaml --in_scp data/train/wav.scp \
        --out_cmvn data/train/global_cmvn

Reads ``dataset_conf.feats_type``, ``dataset_conf.{type}_conf.num_mel_bins`` and an optional
``dataset_conf.resample_conf.resample_rate`` as the reference does (:109-116), serves plain and segmented entries
(``path`` or ``path,start,end`` in seconds, :38-45), and writes ``{"mean_stat", "var_stat", "frame_num"}`` (:144-151).
Utterances are grouped by sample rate into zero-padded batches in file order; a batch goes Resample -> Fbank(window="povey")
or Mfcc -> CmvnStats.update, with the frames of each row from Fbank.num_frames of its own length.  The sums are in double
(wekws_amd/cmvn.py).  Wavs are read with the standard library's ``wave``: 16-bit PCM only, first channel."""
import argparse
import codecs
import sys
import wave

import numpy as np
import torch
import yaml

from wekws_amd.cmvn import CmvnStats
from wekws_amd.frontend import Fbank, Mfcc, Resample

BATCH = 64


def read_scp(path):
    """[(key, wav path, start seconds or None, end seconds or None)] of a wav.scp (:79-82, :31-33)"""
    items = []
    with codecs.open(path, "r", encoding="utf-8") as f:
        for line in f:
            arr = line.strip().split()
            if not arr:
                continue
            value = arr[1].strip().split(",")
            if len(value) not in (1, 3):
                raise SystemExit(f"{path}: '{arr[1]}' is neither a path nor path,start,end")
            items.append((arr[0], value[0], float(value[1]) if len(value) == 3 else None, float(value[2]) if len(value) == 3 else None))
    return items


def read_wav(path, start=None, end=None):
    """(first channel as int16, sample rate); start / end in seconds cut as torchaudio.load(frame_offset, num_frames) does"""
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2 or w.getcomptype() != "NONE":
            raise SystemExit(f"{path}: {8 * w.getsampwidth()}-bit {w.getcomptype()} samples: only 16-bit PCM wavs are read here")
        rate, channels, total = w.getframerate(), w.getnchannels(), w.getnframes()
        first, count = 0, total
        if start is not None:
            first = int(start * rate)
            count = int(end * rate) - first
        first = min(max(first, 0), total)
        count = min(max(count, 0), total - first)
        w.setpos(first)
        pcm = np.frombuffer(w.readframes(count), dtype="<i2").reshape(-1, channels)[:, 0]
    return np.ascontiguousarray(pcm, dtype=np.int16), rate


def feature_batches(items, feat_type, feat_dim, resample_rate=0, device="cuda", batch=BATCH):
    """Yields (feats (B, T, feat_dim) on the device, frames per row) for the utterances of ``items`` (read_scp's), grouped by
    sample rate in order of first appearance, ``batch`` utterances at a time in file order."""
    if feat_type not in ("fbank", "mfcc"):
        raise SystemExit(f"feats_type '{feat_type}': fbank or mfcc")
    by_rate = {}
    for _, path, start, end in items:
        pcm, rate = read_wav(path, start, end)
        by_rate.setdefault(rate, []).append(pcm)
    for rate, rows in by_rate.items():
        out_rate = resample_rate if resample_rate not in (0, rate) else rate
        resample = Resample(rate, out_rate, device=device) if out_rate != rate else None
        front = Fbank(feat_dim, out_rate, window="povey", device=device) if feat_type == "fbank" else \
            Mfcc(feat_dim, feat_dim, out_rate, device=device)
        num_frames = (front if feat_type == "fbank" else front.fbank).num_frames
        for at in range(0, len(rows), batch):
            group = rows[at:at + batch]
            lens = [int(r.size) for r in group]
            pcm = np.zeros((len(group), max(lens + [1])), dtype=np.int16)
            for i, r in enumerate(group):
                pcm[i, :r.size] = r
            x = torch.from_numpy(pcm).to(device)
            if resample is not None:
                x, lens = resample(x, lens)                  # float32 in int16 scale, zeros past a row's own count
            else:
                x = x.to(torch.float32)                      # waveform * (1 << 15) of the reference (:49)
            yield front(x), [num_frames(n) for n in lens]


def main(argv=None):
    ap = argparse.ArgumentParser(description="extract CMVN stats")
    ap.add_argument("--num_workers", default=0, type=int, help="accepted for the reference's command lines; ignored")
    ap.add_argument("--train_config", default="", help="training yaml conf")
    ap.add_argument("--in_scp", default=None, help="wav scp file")
    ap.add_argument("--out_cmvn", default="global_cmvn", help="global cmvn file")
    args = ap.parse_args(argv)
    with open(args.train_config, "r") as fin:
        configs = yaml.load(fin, Loader=yaml.FullLoader)
    feat_type = configs["dataset_conf"]["feats_type"]
    feat_dim = configs["dataset_conf"][f"{feat_type}_conf"]["num_mel_bins"]
    resample_rate = 0
    if "resample_conf" in configs["dataset_conf"]:
        resample_rate = configs["dataset_conf"]["resample_conf"]["resample_rate"]
        print("using resample and new sample rate is {}".format(resample_rate))
    stats = CmvnStats(feat_dim)
    wavs = 0
    for feats, frames in feature_batches(read_scp(args.in_scp), feat_type, feat_dim, resample_rate):
        stats.update(feats, frames)
        wavs += len(frames)
    stats.save(args.out_cmvn)
    print(f"processed {wavs} wavs, {stats.result()['frame_num']} frames", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
