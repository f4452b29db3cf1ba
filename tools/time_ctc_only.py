#!/usr/bin/env python3
"""The CTC-only forward (mdd_create_ctc) beside the attention forward with the same acoustic weights, at the benchmark's shapes:

    B = 64 and 512 utterances of T' = 250 posterior frames (T = 500 stacked frames), H = 384 and H = 256 in mode f32x6, H = 384 in mode f32;
    the attention handle with L = 40 canonical phonemes.

Per configuration, through mdd_forward_profile (each stage replayed alone between two HIP events) and through whole forwards:

    ctc_tail_ms        the ctc_tail stage: median of --reps profiles after --warmup untimed ones
    ctc_tail_GBps      its bytes (R 2H 4 read + R C 4 written, R = T' B) over that time
    attn_tail_ms       the attn_tail stage of the attention handle, the same way, in the same process on the same card, interleaved
    forward_ms         whole forwards (graph replays) of either handle: --reps between two events, after --warmup; alternating the two handles
                       over --rounds rounds, the median round reported

ctc_tail does a subset of attn_tail's work (half the classifier's K, no softmax over L, no context product), and the CTC-only forward a
subset of the attention forward's stages, so ctc_tail <= attn_tail and forward(CTC-only) <= forward(attention) are expected at every shape;
"holds" says whether they were measured so.  Prints one JSON line per configuration and, with --out, writes the notes file.

Usage:  python tools/time_ctc_only.py [--reps 10] [--warmup 3] [--rounds 3] [--only 0,1,..] [--out profiles/ctc_only_notes.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = ((64, 384, "f32x6"), (512, 384, "f32x6"), (64, 256, "f32x6"), (512, 256, "f32x6"), (64, 384, "f32"), (512, 384, "f32"))
TP, L = 250, 40


def stage_ms(model, x, x1, stage, reps, warmup):
    vals = []
    for i in range(warmup + reps):
        ms = dict((p[0], p[1]) for p in model.profile(x, x1))[stage]
        if i >= warmup:
            vals.append(ms)
    return statistics.median(vals), min(vals), max(vals)


def forward_ms(model, x, x1, reps, warmup):
    import torch
    out = None
    for _ in range(warmup):
        out = model.forward(x, x1, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        model.forward(x, x1, out=out)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    from tests import ctc_only_cases as cc
    if not torch.cuda.is_available():
        sys.exit("time_ctc_only: no GPU; a time is measured on the MI355X or not at all")
    only = None if a.only is None else {int(v) for v in a.only.split(",")}
    lines = []
    for n, (B, H, mode) in enumerate(CONFIGS):
        if only is not None and n not in only:
            continue
        geom = cc.geometry(dict(hidden=H))
        sd = synth.synth_state_dict(geom, seed=1234)
        ageom, asd = cc.attention_twin(geom, sd, seed=1234)
        x = torch.from_numpy(synth.synth_batch(ageom, B=B, T=2 * TP, L=L, seed=5)[0]).cuda()
        x1 = torch.from_numpy(synth.synth_batch(ageom, B=B, T=2, L=L, seed=5)[1]).cuda()
        mc, ma = HipModel(geom, sd, precision=mode), HipModel(ageom, asd, precision=mode)
        assert mc.precision == ma.precision == mode
        ct, at = [], []
        for _ in range(a.rounds):        # the two handles alternate: a drift of the card's clock falls on both
            ct.append(stage_ms(mc, x, None, "ctc_tail", a.reps, a.warmup))
            at.append(stage_ms(ma, x, x1, "attn_tail", a.reps, a.warmup))
        fc, fa = [], []
        for _ in range(a.rounds):
            fc.append(forward_ms(mc, x, None, a.reps, a.warmup))
            fa.append(forward_ms(ma, x, x1, a.reps, a.warmup))
        R = TP * B
        nbytes = R * 2 * H * 4 + R * geom.num_class * 4
        c_ms, a_ms = statistics.median(v[0] for v in ct), statistics.median(v[0] for v in at)
        res = dict(B=B, Tp=TP, H=H, mode=mode, L_attention=L, rows=R, ctc_tail_ms=c_ms, ctc_tail_ms_min=min(v[1] for v in ct), ctc_tail_ms_max=max(v[2] for v in ct),
                   ctc_tail_bytes=nbytes, ctc_tail_GBps=nbytes / (c_ms * 1e-3) / 1e9, ctc_tail_GFLOPs=2.0 * R * 2 * H * geom.num_class / (c_ms * 1e-3) / 1e9,
                   attn_tail_ms=a_ms, attn_tail_ms_min=min(v[1] for v in at), attn_tail_ms_max=max(v[2] for v in at),
                   forward_ctc_only_ms=statistics.median(fc), forward_ctc_only_rounds=fc, forward_attention_ms=statistics.median(fa), forward_attention_rounds=fa,
                   holds=dict(tail=c_ms <= a_ms, forward=statistics.median(fc) <= statistics.median(fa)),
                   device=torch.cuda.get_device_name(0), compute_units=torch.cuda.get_device_properties(0).multi_processor_count)
        mc.close(); ma.close()
        del x, x1
        torch.cuda.empty_cache()
        line = json.dumps(res, sort_keys=True)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/time_ctc_only.py --reps %d --warmup %d --rounds %d: one JSON line per configuration (see the tool's docstring for the fields)\n"
                    % (a.reps, a.warmup, a.rounds))
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
