#!/usr/bin/env python3
"""What the wide beam search costs: mdd_beam_wide beside mdd_beam_nbest where both accept the shape, and alone beyond -- on the inputs of
tools/time_nbest.py (B = 64 and 512 utterances of T = 250 posterior frames, C = 45, lm_alpha 0, peaky posteriors with 40 peaks per
utterance; every call at nbest = 1).

  both entries, the same build, the two alternating call by call:   beam 10, 16 (the single-wave kernel) and 64 (the generic kernel)
  mdd_beam_wide alone:                                              beam 65, 100, 200, 256
  one long utterance (B = 1), mdd_beam_wide alone:                  (beam 64, T 664) and (beam 20, T 3500), peaks every 8 frames

Every call is timed on its own between two HIP events, after --warmup untimed calls of that entry at that shape; the calls of a shape
are enqueued back to back and the stream is waited for once at the end, so an interval holds the device's work for the call (its frame
pre-pass and its stream-ordered scratch included) and no idle gap.  The figure is the median of --reps >= 20 calls, the minimum and
maximum ride along.  Before it is timed, every shape both entries take is checked to give the same bits from both, and every wide call
to end with status 0.  One JSON line per run; --out writes the table as well (the head and the last line of
profiles/beam_wide_notes.txt are such a file; the reading between them is written by hand).

Usage:  python tools/time_beam_wide.py [--B 64 512] [--reps 30] [--warmup 5] [--out profiles/beam_wide_table.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, CN = 250, 45
BOTH, WIDE_ONLY, LONG = (10, 16, 64), (65, 100, 200, 256), ((64, 664), (20, 3500))


def timed_pair(fns, reps, warmup):
    """{name: stats} of the entries in ``fns`` (name -> call), alternating call by call in one stream."""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in fns}
    for i in range(reps):
        for k, fn in fns.items():
            e0, e1 = ev[k][i]
            e0.record()
            fn()
            e1.record()
    torch.cuda.synchronize()
    out = {}
    for k in fns:
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev[k])
        out[k] = dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])
    return out


def run(B, Tn, peaks, beams, both, reps, warmup):
    import numpy as np
    import torch
    from ctc_attention_mispronunciation_amd import _lib, synth
    from ctc_attention_mispronunciation_amd.utils.NgramLM import LanguageModel
    lp = torch.from_numpy(np.stack([synth.peaky_logp(Tn, CN, peaks, seed=9000 + b) for b in range(B)], axis=1)).cuda()
    lens = torch.full((B,), Tn, dtype=torch.int32, device="cuda")
    table = LanguageModel(arpa_file=os.path.join(ROOT, "tests", "golden", "lm_synth45.arpa")).dense_table(synth.phone_table_41(), CN)
    lm = torch.from_numpy(table).cuda()
    L, st, p = _lib.lib(), _lib.current_stream_ptr(), (lambda t: C.c_void_p(t.data_ptr()))
    out = {k: (torch.empty((B, Tn), dtype=torch.int32, device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda"),
               torch.empty((B,), dtype=torch.int32, device="cuda"), torch.empty((B,), dtype=torch.float64, device="cuda")) for k in ("nbest", "wide")}
    rows = []
    for beam in beams:
        def nbest(beam=beam):
            ids, nids, status, score = out["nbest"]
            _lib.check(L.mdd_beam_nbest(p(lp), Tn, B, CN, p(lens), beam, 0, p(lm), 0.0, 1, p(ids), p(nids), p(status), p(score), st))

        def wide(beam=beam):
            ids, nids, status, score = out["wide"]
            _lib.check(L.mdd_beam_wide(p(lp), Tn, B, CN, p(lens), beam, 0, p(lm), 0.0, 1, p(ids), p(nids), p(status), p(score), None, 0, st))

        fns = dict(mdd_beam_nbest=nbest, mdd_beam_wide=wide) if both else dict(mdd_beam_wide=wide)
        for t in out.values():
            t[0].fill_(-1)
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        assert not out["wide"][2].any().item(), "a timing input must decode without an error status"
        if both:
            assert all(torch.equal(a, b) for a, b in zip(out["nbest"], out["wide"])), "the two entries differ at beam %d" % beam
        row = dict(B=B, T=Tn, beam=beam, longest=int(out["wide"][1].max().item()))
        row.update(timed_pair(fns, reps, warmup))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: the median needs at least 20 calls")
    rows = []
    for B in a.B:
        rows += run(B, T, 40, BOTH, True, a.reps, a.warmup)
        rows += run(B, T, 40, WIDE_ONLY, False, a.reps, a.warmup)
    for beam, Tn in LONG:
        rows += run(1, Tn, Tn // 8, (beam,), False, a.reps, a.warmup)
    res = dict(C=CN, reps=a.reps, warmup=a.warmup, rows=rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        def cell(r, k):
            return "%8.4f [%8.4f .. %8.4f]" % (r[k]["median_ms"], r[k]["min_ms"], r[k]["max_ms"]) if k in r else "%30s" % "-"
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("Wide beam search (tools/time_beam_wide.py): C = %d, peaky posteriors, nbest 1; ms per call between HIP events, median [min .. max]\n"
                    "of %d warm calls, back to back, the two entries of a row alternating\n" % (CN, a.reps))
            f.write("%5s %5s %5s %8s  %-30s  %-30s  %s\n" % ("B", "T", "beam", "longest", "mdd_beam_nbest", "mdd_beam_wide", "wide / nbest"))
            for r in rows:
                ratio = "%.2f" % (r["mdd_beam_wide"]["median_ms"] / r["mdd_beam_nbest"]["median_ms"]) if "mdd_beam_nbest" in r else "-"
                f.write("%5d %5d %5d %8d  %s  %s  %s\n" % (r["B"], r["T"], r["beam"], r["longest"], cell(r, "mdd_beam_nbest"), cell(r, "mdd_beam_wide"), ratio))
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
