#!/usr/bin/env python3
"""Front end to the padded model input, B utterances of S seconds (default: 64 x 10 s, the bench workload's shape), timed
two ways in one process on the MI355X:

  batched         one fbank_batch launch (mdd_fbank_batch): WAVs -> [B, T_out, 243] padded batch
  per-utterance   per utterance mdd_fbank + mdd_stack_skip, then a copy into the padded batch (and a zero fill of it)

Samples are on the device already in both routes (the host -> device copy is outside the timing).  Median of --reps
HIP-event intervals after --warmup untimed runs.  Prints one JSON line; --out also writes it to a file.

Usage:  python tools/fbank_batch_time.py [--B 64] [--seconds 10] [--reps 50] [--warmup 5] [--out PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ctc_attention_mispronunciation_amd import _lib  # noqa: E402
from ctc_attention_mispronunciation_amd.utils import fbank as fb  # noqa: E402
from ctc_attention_mispronunciation_amd.utils.data_loader import stack_features  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    n = int(a.seconds * 16000)
    rs = np.random.default_rng(0)
    wav = torch.from_numpy((rs.standard_normal(a.B * n) * 3000).astype(np.float32)).cuda()
    offs = torch.arange(0, (a.B + 1) * n, n, dtype=torch.int64).cuda()
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(ROOT, "tests", "golden", "global_fbank_cmvn.txt")))
    sc, of = torch.from_numpy(cmvn[0]).cuda(), torch.from_numpy(cmvn[1]).cuda()
    lens = np.full(a.B, n, dtype=np.int64)
    T_out = L.mdd_fbank_batch_len(lens.ctypes.data_as(C.POINTER(C.c_int64)), a.B, 2, 2)
    T_raw = L.mdd_fbank_num_frames(n)
    out = torch.empty((a.B, T_out, 243), dtype=torch.float32, device="cuda")
    raw = torch.empty((a.B, T_raw, 81), dtype=torch.float32, device="cuda")
    out2 = torch.empty_like(out)
    st = _lib.current_stream_ptr()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def batched():
        _lib.check(L.mdd_fbank_batch(p(wav), p(offs), a.B, T_out, p(sc), p(of), 2, 2, 2, p(out), st))

    def per_utterance():
        out2.zero_()
        for b in range(a.B):
            _lib.check(L.mdd_fbank(C.c_void_p(wav.data_ptr() + 4 * b * n), n, p(sc), p(of), p(raw[b]), st))
            x = stack_features(raw[b])
            out2[b, :x.shape[0]].copy_(x)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    tb, tb_min = timed(batched)
    tp, tp_min = timed(per_utterance)
    torch.cuda.synchronize()
    same = bool(torch.equal(out, out2))
    moved = a.B * n * 4 + out.numel() * 4
    res = dict(B=a.B, seconds=a.seconds, T_out=T_out, batched_ms=tb, batched_min_ms=tb_min, per_utterance_ms=tp,
               per_utterance_min_ms=tp_min, batched_GBps=moved / tb / 1e6, bytes_moved=moved, identical=same)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
