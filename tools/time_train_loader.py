#!/usr/bin/env python3
"""Training batches of B utterances of S seconds (default 32 x 10 s, the training step's workload), timed per batch on the two input
routes, in one process on the MI355X:

  wav   TrainWavLoader(train=True): host draws + one copy of the samples + one mdd_fbank_batch_aug launch.  Host wall time per
        batch (until the batch is complete on the device) and GPU time per batch (HIP events around the batch's work).
        With --speeds the batch also passes mdd_resample_batch.
  ark   SpeechDataLoader(SpeechDataset(train=True)) over the same utterances' features in a Kaldi ark: file read, spec_augment,
        make_context, skip, pad and collate per item on the host, then the copy of the padded batch to the device.  Wall time per
        batch with num_workers 0 and --workers (default 8; never sized by the machine's CPU count).

The yardsticks are the ark route and the training step (profiles/train_f32x6_notes.txt: 14.3 ms bf16x3, 25.7 ms f32x6, 32.7 ms f32
per 32-utterance step).  Prints one JSON line; --out also writes it to a file.

Usage:  python tools/time_train_loader.py [--B 32] [--seconds 10] [--batches 6] [--workers 8] [--speeds 0.9,1.0,1.1] [--out PATH]
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ctc_attention_mispronunciation_amd.synth import phone_table_41  # noqa: E402
from ctc_attention_mispronunciation_amd.utils import fbank as fb  # noqa: E402
from ctc_attention_mispronunciation_amd.utils.data_loader import SpeechDataLoader, SpeechDataset, TrainWavLoader, Vocab  # noqa: E402

STEPS_MS = {"bf16x3": 14.3, "f32x6": 25.7, "f32": 32.7}


def per_batch(loader, device_copy):
    """Wall ms per batch of one pass, each batch complete on the device; the first batch (start-up of workers) apart."""
    stamps = [time.perf_counter()]
    for batch in loader:
        if device_copy:
            batch[0].cuda()
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
    ms = np.diff(stamps) * 1e3
    return dict(first_ms=float(ms[0]), median_ms=float(np.median(ms[1:])), max_ms=float(ms[1:].max()), batches=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--speeds", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    random.seed(0), np.random.seed(0), torch.manual_seed(0)
    n, count = int(a.seconds * 16000), a.B * a.batches
    rs = np.random.default_rng(0)
    i2c = phone_table_41()
    phones = [i2c[i] for i in range(3, 44)]
    utts = ["utt%04d" % i for i in range(count)]
    wavs = [np.rint(rs.standard_normal(n) * 3000).astype(np.float32) for _ in range(count)]
    can = [" ".join(rs.choice(phones, size=40)) for _ in range(count)]
    lab = [" ".join(rs.choice(phones, size=40)) for _ in range(count)]
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(ROOT, "tests", "golden", "global_fbank_cmvn.txt")))
    res = dict(B=a.B, seconds=a.seconds, batches=a.batches, steps_ms=STEPS_MS)
    with tempfile.TemporaryDirectory() as tmp:
        units = os.path.join(tmp, "units")
        with open(units, "w") as f:
            f.write("".join(i2c[i] + "\n" for i in range(2, len(i2c))))
        vocab = Vocab(units)
        # ---- the WAV route
        speeds = [float(s) for s in a.speeds.split(",")] if a.speeds else None
        loader = TrainWavLoader(list(zip(utts, wavs, can, lab)), vocab, a.B, cmvn=cmvn, train=True, shuffle=True, speeds=speeds)
        next(iter(loader))                                   # tables, first launches
        torch.cuda.synchronize()
        wall, gpu = [], []
        it = iter(loader)
        for _ in range(len(loader)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            next(it)
            e1.record()
            e1.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            gpu.append(e0.elapsed_time(e1))
        res["wav"] = dict(wall_median_ms=float(np.median(wall)), wall_max_ms=float(np.max(wall)), gpu_median_ms=float(np.median(gpu)),
                          gpu_min_ms=float(np.min(gpu)), speeds=speeds)
        # the statistics pass over the same set (once per corpus, in front of the first epoch)
        t0 = time.perf_counter()
        stats = fb.cmvn_stats(wavs, batch_size=a.B)
        res["cmvn_stats_ms_per_batch"] = (time.perf_counter() - t0) * 1e3 / a.batches
        res["cmvn_frames"] = int(stats[0, 81])
        # ---- the ark route over the same utterances
        feats = {}
        for start in range(0, count, a.B):                   # features through the batched front end: the same bits, fewer launches
            x, _ = fb.fbank_batch(wavs[start:start + a.B], cmvn=cmvn, right_ctx=0, n_skip_frame=1, n_downsample=1)
            for k, u in enumerate(utts[start:start + a.B]):
                feats[u] = x[k].cpu().numpy()
        fb.write_ark_scp(os.path.join(tmp, "fbank.ark"), os.path.join(tmp, "fbank.scp"), feats)
        del feats
        for name, rows in (("lab", lab), ("trans", can)):
            with open(os.path.join(tmp, name), "w") as f:
                f.write("".join("%s %s\n" % p for p in zip(utts, rows)))
        opts = types.SimpleNamespace(left_ctx=0, right_ctx=2, n_skip_frame=2, n_downsample=2)
        ds = SpeechDataset(vocab, os.path.join(tmp, "fbank.scp"), os.path.join(tmp, "lab"), os.path.join(tmp, "trans"), opts, train=True)
        for workers in (0, a.workers):
            # (workers are spawned, not forked: a child of a process that has the GPU open must not inherit it)
            kw = dict(multiprocessing_context="spawn") if workers else {}
            res["ark_workers%d" % workers] = per_batch(SpeechDataLoader(ds, batch_size=a.B, shuffle=True, num_workers=workers, **kw), True)
    for route in ("wav", "ark_workers0", "ark_workers%d" % a.workers):
        ms = res[route]["wall_median_ms"] if route == "wav" else res[route]["median_ms"]
        res[route]["keeps_up_with"] = {k: bool(ms <= v) for k, v in STEPS_MS.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
