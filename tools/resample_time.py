#!/usr/bin/env python3
"""Any-rate front end, B utterances of S seconds at 44.1 and 48 kHz (default: 64 x 10 s, the bench workload's shape), timed in
one process on the MI355X:

  resample            one resample_batch launch (mdd_resample_batch): B ragged rows -> 16 kHz PCM16 samples on the device
  resample + fbank    the same, then one fbank_batch launch (mdd_fbank_batch) on the device samples -> [B, T_out, 243]
  oracle              the float64 numpy restatement of the resampler (tests/test_resample.py) on the host, for --oracle_rows rows
                      (scaled to B rows), to set the GPU numbers against

Samples, offsets and rates are on the device already (the host -> device copy is outside the timing).  mdd_resample_batch
reads its offsets and rates back to size its launch, and that sync is inside the timing.  Median of --reps HIP-event intervals
after --warmup untimed runs.  The first row of each rate is checked bit for bit against the oracle.  Prints one JSON line;
--out also writes it to a file.

Usage:  python tools/resample_time.py [--B 64] [--seconds 10] [--reps 20] [--warmup 3] [--oracle_rows 1] [--out PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ctc_attention_mispronunciation_amd import _lib  # noqa: E402
from ctc_attention_mispronunciation_amd.utils import fbank as fb  # noqa: E402
from tests.test_resample import restate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--oracle_rows", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(ROOT, "tests", "golden", "global_fbank_cmvn.txt")))
    sc, of = torch.from_numpy(cmvn[0]).cuda(), torch.from_numpy(cmvn[1]).cuda()
    st = _lib.current_stream_ptr()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    res = dict(B=a.B, seconds=a.seconds, reps=a.reps)
    ok = True
    for rate in (44100, 48000):
        n = int(a.seconds * rate)
        rs = np.random.default_rng(rate)
        host = (rs.standard_normal(a.B * n) * 3000).astype(np.float32)
        wav = torch.from_numpy(host).cuda()
        n16 = fb.resample_len(n, rate)
        in_off = torch.arange(0, (a.B + 1) * n, n, dtype=torch.int64).cuda()
        out_off = torch.arange(0, (a.B + 1) * n16, n16, dtype=torch.int64).cuda()
        rates = torch.full((a.B,), rate, dtype=torch.int32).cuda()
        y = torch.empty(a.B * n16, dtype=torch.float32, device="cuda")
        lens = np.full(a.B, n16, dtype=np.int64)
        T_out = L.mdd_fbank_batch_len(lens.ctypes.data_as(C.POINTER(C.c_int64)), a.B, 2, 2)
        feats = torch.empty((a.B, T_out, 243), dtype=torch.float32, device="cuda")

        def resample():
            _lib.check(L.mdd_resample_batch(p(wav), p(in_off), p(rates), a.B, p(out_off), p(y), st))

        def both():
            resample()
            _lib.check(L.mdd_fbank_batch(p(y), p(out_off), a.B, T_out, p(sc), p(of), 2, 2, 2, p(feats), st))

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

        tr, tr_min = timed(resample)
        tb, tb_min = timed(both)
        torch.cuda.synchronize()
        got = y[:n16].cpu().numpy()
        t0 = time.time()
        for r in range(a.oracle_rows):
            want = restate(host[r * n:(r + 1) * n], rate)
        oracle_row_s = (time.time() - t0) / a.oracle_rows
        same = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        ok &= same
        step = int(min(1.0, 16000.0 / rate) * 512)
        taps = 2 * (32769 // step)                      # upper bound of taps per output (both wings)
        res[str(rate)] = dict(n_in=n, n_out=n16, T_out=T_out, resample_ms=tr, resample_min_ms=tr_min, resample_fbank_ms=tb,
                              resample_fbank_min_ms=tb_min, oracle_row_s=oracle_row_s, oracle_batch_s_est=oracle_row_s * a.B,
                              taps_per_output_max=taps, tap_products_G=a.B * n16 * taps / 1e9,
                              table_bytes_per_tap=16, identical_to_oracle_row0=same)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
