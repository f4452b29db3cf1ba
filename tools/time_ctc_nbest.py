#!/usr/bin/env python3
"""What rescoring an N-best list costs: mdd_ctc_nbest (all ranks in one launch, csrc/ctc_nbest.hip) against the route it replaces, one
mdd_ctc_loss call without gradient per rank, in the same process on the same posteriors and lists.

Shapes (B, N, T, max_len) at C = 45: (64, 10, 250, 64), (64, 200, 250, 64), (512, 10, 250, 64), (64, 1, 250, 64), (64, 200, 600, 255).
The posteriors are peaky ones (synth.peaky_logp, 40 peaks), the lists tests/mbr_reference.draw_lists' (a base sequence of max_len / 2 ..
max_len ids and 0-3 edits per rank, no blank), as tools/time_mbr.py times them.  Per shape:

  entry        hip_model.ctc_nbest: the launch, its output from torch's allocator; device work only
  loop         hip_model.ctc_loss(want_grad=False) per rank, as BeamDecoder.nbest_loglik ran it; device work only
  nbest_loglik BeamDecoder.nbest_loglik as it routes now, ending in the copy to the host (what tools/time_mbr.py calls `rescore`)
  loop_loglik  the same with hip_model.ctc_nbest_fits refusing: the parent's nbest_loglik
  sweep        entry under MDD_CTC_NBEST_WAVES x MDD_CTC_NBEST_HPB: the table behind ctc_nbest_plan's choice (csrc/plan.h)

Before anything is timed the entry's bits are compared with the loop's.  Every call is timed on its own between two HIP events after
--warmup untimed calls; the figure is the median of --reps calls with the minimum and maximum beside it.  The LDS of a workgroup and the
workgroups a CU holds (the smaller of 160 KiB / LDS and 32 waves / waves per workgroup) are printed per shape.  One JSON line per run;
--out writes the notes file as well.

Usage:  python tools/time_ctc_nbest.py [--reps 30] [--warmup 5] [--out profiles/ctc_nbest_notes.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CN = 45
SHAPES = ((64, 10, 250, 64), (64, 200, 250, 64), (512, 10, 250, 64), (64, 1, 250, 64), (64, 200, 600, 255))
SWEEP_WAVES = (2, 4, 8, 16)
SWEEP_HPB = (2, 4, 5, 8, 10, 16, 32)
SWITCHES = ("MDD_CTC_NBEST_WAVES", "MDD_CTC_NBEST_HPB")


def timed(fn, reps, warmup, sync_each=False):
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
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def run(B, N, T, max_len, reps, warmup, sweep):
    import numpy as np
    import torch
    from ctc_attention_mispronunciation_amd import hip_model, synth
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    from tests import ctc_nbest_cases as cc
    from tests import mbr_reference as mr
    for var in SWITCHES:
        os.environ.pop(var, None)
    ids_h, nids_h = mr.draw_lists(4000 + B + N + max_len, N, B, CN, max_len, pitch=max_len)
    lp = torch.from_numpy(np.stack([synth.peaky_logp(T, CN, 40, seed=9000 + b) for b in range(B)], axis=1)).cuda()
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    ids = torch.zeros((N, B, T), dtype=torch.int32, device="cuda")
    ids[:, :, :max_len] = torch.from_numpy(ids_h).cuda().clamp(min=1)          # the list as labels: no blank
    nids = torch.from_numpy(nids_h).cuda()
    assert hip_model.ctc_nbest_fits(T, CN, max_len)
    p = cc.plan(T, B, CN, N, max_len)
    res = dict(B=B, N=N, T=T, max_len=max_len, mean_len=float(nids_h.mean()), waves=p.waves, hyps_per_block=p.hyps_per_block, NL=p.NL,
               lds_bytes=p.smem, grid=[p.groups, B], workgroups_per_cu=min(160 * 1024 // p.smem, 32 // p.waves))

    def entry():
        return hip_model.ctc_nbest(lp, lens, ids, nids, max_len=max_len)

    def loop():
        return [hip_model.ctc_loss(lp, ids[n, :, :max_len], lens, nids[n], want_grad=False)[0] for n in range(N)]

    same = (-entry()).float().view(torch.int32) == torch.stack(loop()).view(torch.int32)
    assert bool(same.all()), "the entry's bits differ from the loop's"
    res["finite_share"] = float(torch.isfinite(entry()).double().mean())
    few = max(reps // 4, 8) if N >= 100 else reps
    res["entry"] = timed(entry, reps, warmup)
    res["loop"] = timed(loop, few, 2)
    res["entry_again"] = timed(entry, reps, warmup)           # the two arms alternate: the spread between the entry's two windows
    dec = BeamDecoder(synth.phone_table_41(), beam_width=max(N, 2), blank_index=0, space_idx=-1,
                      lm_path=os.path.join(ROOT, "tests", "golden", "lm_synth45.arpa"), lm_alpha=0.0)
    res["nbest_loglik"] = timed(lambda: dec.nbest_loglik(lp, lens, ids, nids, max_len=max_len), reps, warmup, True)
    fits = hip_model.ctc_nbest_fits
    hip_model.ctc_nbest_fits = lambda *a: False
    try:
        res["loop_loglik"] = timed(lambda: dec.nbest_loglik(lp, lens, ids, nids, max_len=max_len), few, 2, True)
    finally:
        hip_model.ctc_nbest_fits = fits
    if sweep:
        res["sweep"] = {}
        for w in SWEEP_WAVES:
            for h in SWEEP_HPB:
                os.environ["MDD_CTC_NBEST_WAVES"], os.environ["MDD_CTC_NBEST_HPB"] = str(w), str(h)
                res["sweep"]["%dx%d" % (w, h)] = timed(entry, reps, warmup)["median_ms"]
        for var in SWITCHES:
            os.environ.pop(var, None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", type=int, nargs="+", default=list(range(len(SHAPES))), help="indices into SHAPES")
    ap.add_argument("--no_sweep", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: the median needs at least 20 calls")
    res = dict(C=CN, reps=a.reps, warmup=a.warmup, shapes=[run(*SHAPES[i], a.reps, a.warmup, not a.no_sweep) for i in a.shapes])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("Rescoring an N-best list (tools/time_ctc_nbest.py): C = %d, peaky posteriors, lists of a base sequence with 0-3 edits per rank;\n"
                    "ms per call between HIP events, median [min .. max] of %d warm calls (the loops at N >= 100: %d calls).  The entry's bits were\n"
                    "compared with the loop's at every shape before timing.\n" % (CN, a.reps, max(a.reps // 4, 8)))
            for s in res["shapes"]:
                f.write("B = %d, N = %d, T = %d, max_len = %d (mean length %.1f ids, %.0f %% of the rows CTC paths): %d waves, %d ranks per workgroup, NL = %d,\n"
                        "  grid %d x %d, LDS %d bytes per workgroup, %d workgroup(s) per CU\n"
                        % (s["B"], s["N"], s["T"], s["max_len"], s["mean_len"], 100 * s["finite_share"], s["waves"], s["hyps_per_block"], s["NL"],
                           s["grid"][0], s["grid"][1], s["lds_bytes"], s["workgroups_per_cu"]))
                for k, label in (("entry", "mdd_ctc_nbest"), ("entry_again", "mdd_ctc_nbest, second window"), ("loop", "mdd_ctc_loss per rank"),
                                 ("nbest_loglik", "nbest_loglik (to the host)"), ("loop_loglik", "nbest_loglik by the loop (to the host)")):
                    v = s[k]
                    f.write("  %-40s %10.4f  [%.4f .. %.4f]\n" % (label, v["median_ms"], v["min_ms"], v["max_ms"]))
                f.write("  loop / entry %.1fx on the device, %.1fx to the host\n"
                        % (s["loop"]["median_ms"] / s["entry"]["median_ms"], s["loop_loglik"]["median_ms"] / s["nbest_loglik"]["median_ms"]))
                if "sweep" in s:
                    f.write("  sweep, median ms of the entry (waves x ranks per workgroup):\n")
                    for w in SWEEP_WAVES:
                        cells = ["%dx%-3d %8.4f" % (w, h, s["sweep"]["%dx%d" % (w, h)]) for h in SWEEP_HPB if "%dx%d" % (w, h) in s["sweep"]]
                        f.write("    " + "   ".join(cells) + "\n")
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
