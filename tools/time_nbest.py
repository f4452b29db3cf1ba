#!/usr/bin/env python3
"""What the N-best ending of the beam search costs: mdd_beam beside mdd_beam_nbest at N = 1, 5 and 10, and the N slices of rescoring
(BeamDecoder.nbest_loglik: one mdd_ctc_loss without gradient per slice), at the benchmark's decode shape -- B = 64 and B = 512 utterances
of T = 250 posterior frames, C = 45, beam 10, lm_alpha 0, peaky posteriors (synth.peaky_logp, 40 peaks per utterance).

Every call is timed on its own between two HIP events, after --warmup untimed calls; the figure is the median of --reps >= 20 calls (the
minimum and maximum ride along, and the JSON line keeps every sample).  The beam calls are enqueued back to back (--sync_each: the device
idles before each call, see ``timed``).  A beam call includes its frame pre-pass and its stream-ordered scratch; a rescoring call
ends in the copy of the N x B log-likelihoods to the host, so those always wait.  One JSON line per run; --out writes the notes file as well.

--steps beam times mdd_beam alone: with MDD_LIB_PATH pointing at a build of another commit this is the comparison across commits
(mdd_beam launches the instantiation whose ending is the winner-only code, so it must not move).

Usage:  python tools/time_nbest.py [--B 64 512] [--reps 30] [--warmup 5] [--steps beam nbest rescore] [--sync_each]
        [--out profiles/nbest_notes.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, CN, BEAM, NS = 250, 45, 10, (1, 5, 10)


def timed(fn, reps, warmup, sync_each=False):
    """ms of every call between its own pair of HIP events.  By default the calls are enqueued back to back and the stream is waited for
    once at the end, so an interval holds the device's work for the call and no idle gap.  sync_each waits after every call instead: the
    device is idle when a call starts and the interval holds the host's launch path too; at B = 64 such calls fall into two modes
    0.2 ms apart whose shares change from run to run, in any build of the library (profiles/nbest_notes.txt), so medians of that kind
    do not compare builds."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
        if sync_each:
            e1.synchronize()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], ms=[round(v, 4) for v in ms])


def run(B, steps, reps, warmup, sync_each):
    import numpy as np
    import torch
    from ctc_attention_mispronunciation_amd import _lib, synth
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    i2c = synth.phone_table_41()
    dec = BeamDecoder(i2c, beam_width=BEAM, blank_index=0, space_idx=-1, lm_path=os.path.join(ROOT, "tests", "golden", "lm_synth45.arpa"),
                      lm_alpha=0.0)
    lp = torch.from_numpy(np.stack([synth.peaky_logp(T, CN, 40, seed=9000 + b) for b in range(B)], axis=1)).cuda()
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    lm = dec._lm_table(CN, lp.device)
    L, st, p = _lib.lib(), _lib.current_stream_ptr(), (lambda t: C.c_void_p(t.data_ptr()))
    ids = torch.empty((BEAM, B, T), dtype=torch.int32, device="cuda")
    nids = torch.empty((BEAM, B), dtype=torch.int32, device="cuda")
    status = torch.empty((B,), dtype=torch.int32, device="cuda")
    score = torch.empty((BEAM, B), dtype=torch.float64, device="cuda")
    res = dict(B=B)

    def beam():
        _lib.check(L.mdd_beam(p(lp), T, B, CN, p(lens), BEAM, 0, p(lm), 0.0, p(ids), p(nids), p(status), p(score), st))

    def nbest(n):
        _lib.check(L.mdd_beam_nbest(p(lp), T, B, CN, p(lens), BEAM, 0, p(lm), 0.0, n, p(ids), p(nids), p(status), p(score), st))

    if "beam" in steps:
        res["mdd_beam"] = timed(beam, reps, warmup, sync_each)
    if "nbest" in steps:
        for n in NS:
            res["mdd_beam_nbest_N%d" % n] = timed(lambda: nbest(n), reps, warmup, sync_each)
    if "rescore" in steps:
        nbest(BEAM)
        torch.cuda.synchronize()
        assert not status.any().item(), "a timing input must decode without an error status"
        width = int(nids.max().item())
        res["max_ids"] = width
        for n in NS:
            res["rescore_N%d" % n] = timed(lambda: dec.nbest_loglik(lp, lens, ids[:n], nids[:n], max_len=width), reps, warmup, True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", nargs="+", default=["beam", "nbest", "rescore"], choices=["beam", "nbest", "rescore"])
    ap.add_argument("--sync_each", action="store_true", help="wait for the device after every call (see timed)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: the median needs at least 20 calls")
    res = dict(T=T, C=CN, beam=BEAM, reps=a.reps, warmup=a.warmup, lib=os.environ.get("MDD_LIB_PATH", "default"),
               sync_each=a.sync_each,
               shapes=[run(B, a.steps, a.reps, a.warmup, a.sync_each) for B in a.B])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("N-best ending of the beam search (tools/time_nbest.py): T = %d, C = %d, beam %d, peaky posteriors; ms per call between HIP\n"
                    "events, median [min .. max] of %d warm calls%s\n" % (T, CN, BEAM, a.reps, ", the device idle before each" if a.sync_each else ", back to back"))
            for shape in res["shapes"]:
                f.write("B = %d%s\n" % (shape["B"], "  (longest hypothesis: %d ids)" % shape["max_ids"] if "max_ids" in shape else ""))
                for k, v in shape.items():
                    if isinstance(v, dict):
                        f.write("  %-20s %.4f  [%.4f .. %.4f]\n" % (k, v["median_ms"], v["min_ms"], v["max_ms"]))
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
