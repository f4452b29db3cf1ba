#!/usr/bin/env python3
"""What the gradient of the MWER objective costs: mdd_ctc_nbest_grad (all ranks in one call, csrc/ctc_nbest_grad.hip) against the route it
replaces -- N mdd_ctc_loss calls with gradient and the N scaled additions -- in the same process on the same posteriors, lists and
coefficients; then one training step with train.MWERLoss against one with train.CTCLoss at bench.py's train32 shape.

Steps (each a child process of its own under a time limit; the first one that fails or runs out of time ends the run, nothing is tried again):
  grad10, grad100   B = 32, T' = 250, C = 45, hypotheses of about 40 phones (a base sequence of 24..48 ids and 0-3 edits per rank, no blank;
                    tests/mbr_reference.draw_lists), N = 10 and N = 100, coefficients mdd_nbest_risk makes of the list's own log-likelihoods
                    and random costs.  Before anything is timed the entry's output is compared with the loop's.
  train             the step of bench.py's train32 workload (B = 32, T = 500 -> T' = 250, H = 384, exact fp32) with CTCLoss, with MWERLoss
                    (N = 10 of beam 10) and with MWERLoss forced to the per-rank route
Every call is timed on its own between two HIP events after --warmup untimed calls; the figure is the median of --reps calls with the
minimum and maximum beside it.  One JSON line per step; --out writes the notes file as well.

Usage:  python tools/time_ctc_nbest_grad.py [--reps 30] [--warmup 5] [--out profiles/ctc_nbest_grad_notes.txt]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CN, B, T, MAX_LEN = 45, 32, 250, 48
STEPS = {"grad10": 240, "grad100": 420, "train": 420}      # seconds each child may take


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def grad_step(N, reps, warmup):
    import numpy as np
    import torch
    from ctc_attention_mispronunciation_amd import hip_model, synth
    from tests import ctc_nbest_grad_cases as gc
    from tests import mbr_reference as mr
    ids_h, nids_h = mr.draw_lists(6000 + N, N, B, CN, MAX_LEN, pitch=MAX_LEN)
    lp = torch.from_numpy(np.stack([synth.peaky_logp(T, CN, 40, seed=9000 + b) for b in range(B)], axis=1)).cuda()
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    ids = torch.zeros((N, B, T), dtype=torch.int32, device="cuda")
    ids[:, :, :MAX_LEN] = torch.from_numpy(ids_h).cuda().clamp(min=1)          # the list as labels: no blank
    nids = torch.from_numpy(nids_h).cuda()
    cost = torch.from_numpy(np.random.default_rng(6100 + N).integers(0, 12, size=(N, B)).astype(np.int32)).cuda()
    loglik = hip_model.ctc_nbest(lp, lens, ids, nids, max_len=MAX_LEN)
    # the list's own posterior is all but one-hot on such posteriors; flatten it so that every rank is live and the loop has N lattices to run
    post, risk, coef, flag = hip_model.nbest_risk(loglik / 50.0, cost)
    assert not bool(flag.any()) and hip_model.ctc_nbest_grad_fits(T, CN, MAX_LEN)
    p = gc.plan(T, B, CN, N, MAX_LEN)
    res = dict(step="grad%d" % N, B=B, N=N, T=T, C=CN, max_len=MAX_LEN, mean_len=float(nids_h.mean()), live_ranks=float((coef != 0).double().mean()),
               ranks_per_workgroup=p.ranks, grid=[p.groups, B], NL=p.NL, lds_bytes=p.smem, workspace_bytes=p.bytes)

    def entry():
        return hip_model.ctc_nbest_grad(lp, lens, ids, nids, coef, max_len=MAX_LEN)[0]

    def loop():
        total = torch.zeros_like(lp)
        for n in range(N):
            total += coef[n].float().view(1, B, 1) * hip_model.ctc_loss(lp, ids[n, :, :MAX_LEN], lens, nids[n], want_grad=True)[1]
        return total

    a, b_ = entry(), loop()
    bound = 2 * gc.GRAD_ATOL * coef.abs().sum(dim=0).max().item()
    res["entry_minus_loop"] = float((a - b_).abs().max())
    assert res["entry_minus_loop"] <= bound, (res["entry_minus_loop"], bound)
    few = max(reps // 3, 8) if N >= 100 else reps
    res["entry"] = timed(entry, reps, warmup)
    res["loop"] = timed(loop, few, 2)
    res["entry_again"] = timed(entry, reps, warmup)
    return res


def train_step(reps, warmup):
    import numpy as np
    import torch
    import torch.nn as nn
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    from ctc_attention_mispronunciation_amd.steps.train_ctc import build_training
    from ctc_attention_mispronunciation_amd.train import MWERLoss
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    L = 40
    geom = synth.Geometry(feat=243, hidden=384, layers=4, num_class=CN)
    sd = synth.synth_state_dict(geom, seed=1234)
    model = CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=CN, drop_out=0.2)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.cuda().train()
    model.strict_errors = False
    model.train_precision = "f32"
    ctc, opt = build_training(model)
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=2 * T, L=L, seed=1234, ragged=False)
    xd, x1d = torch.from_numpy(x).cuda(), torch.from_numpy(x1).cuda()
    tg = torch.from_numpy(np.random.Generator(np.random.PCG64(7)).integers(2, 44, size=(B, L))).cuda()
    il, tl = torch.full((B,), T, dtype=torch.int64).cuda(), torch.full((B,), L, dtype=torch.int64).cuda()
    dec = BeamDecoder(synth.phone_table_41(), beam_width=10, blank_index=0, space_idx=-1, lm_path=os.path.join(ROOT, "tests", "golden", "lm_synth45.arpa"),
                      lm_alpha=0.0)
    res = dict(step="train", B=B, T=2 * T, hidden=384, nbest=10, beam=10)

    def step_with(loss_fn):
        def step():
            out = model(xd, x1d)
            loss = loss_fn(out, tg, il, tl) / B
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss
        return step

    mwer = MWERLoss(dec, 10)
    res["ctc_step"] = timed(step_with(ctc), reps, warmup)
    res["mwer_step"] = timed(step_with(mwer), reps, warmup)
    res["mwer_fused"] = bool(mwer.last["fused"])
    res["mwer_live_ranks"] = float((mwer.last["coef"] != 0).double().mean())
    res["mwer_flagged"] = int((mwer.last["flag"] != 0).sum())
    res["mwer_per_rank_step"] = timed(step_with(MWERLoss(dec, 10, per_rank=True)), reps, warmup)
    res["ctc_step_again"] = timed(step_with(ctc), reps, warmup)
    return res


def notes(results, reps):
    lines = ["The gradient of the MWER objective (tools/time_ctc_nbest_grad.py): ms per call between HIP events, median [min .. max] of %d warm calls" % reps,
             "(the loop at N = 100: a third of them).  The entry's output was compared with the loop's before timing."]
    for r in results:
        if r["step"].startswith("grad"):
            lines.append("B = %d, N = %d, T' = %d, C = %d, max_len = %d (mean length %.1f ids, %.0f %% of the ranks live): %d rank(s) per workgroup, grid %d x %d, NL = %d,"
                         % (r["B"], r["N"], r["T"], r["C"], r["max_len"], r["mean_len"], 100 * r["live_ranks"], r["ranks_per_workgroup"], r["grid"][0], r["grid"][1], r["NL"]))
            lines.append("  LDS %d bytes per workgroup, workspace %.1f MB; max |entry - loop| %.2e" % (r["lds_bytes"], r["workspace_bytes"] / 1e6, r["entry_minus_loop"]))
            for k, label in (("entry", "mdd_ctc_nbest_grad"), ("entry_again", "mdd_ctc_nbest_grad, second window"), ("loop", "mdd_ctc_loss with gradient per rank + N additions")):
                lines.append("  %-52s %10.4f  [%.4f .. %.4f]" % (label, r[k]["median_ms"], r[k]["min_ms"], r[k]["max_ms"]))
            lines.append("  loop / entry %.1fx" % (r["loop"]["median_ms"] / r["entry"]["median_ms"]))
        else:
            lines.append("One training step, B = %d, T = %d, H = %d, exact fp32 (bench.py's train32), %d-best of beam %d; one-launch route taken: %s;"
                         % (r["B"], r["T"], r["hidden"], r["nbest"], r["beam"], r["mwer_fused"]))
            lines.append("  %.0f %% of the ranks live in the last step, %d utterance(s) flagged" % (100 * r["mwer_live_ranks"], r["mwer_flagged"]))
            for k, label in (("ctc_step", "CTCLoss"), ("ctc_step_again", "CTCLoss, second window"), ("mwer_step", "MWERLoss"), ("mwer_per_rank_step", "MWERLoss, per-rank route forced")):
                lines.append("  %-52s %10.4f  [%.4f .. %.4f]" % (label, r[k]["median_ms"], r[k]["min_ms"], r[k]["max_ms"]))
    return "\n".join(lines) + "\n" + "".join(json.dumps(r) + "\n" for r in results)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", nargs="+", default=list(STEPS), choices=list(STEPS))
    ap.add_argument("--step", default=None, choices=list(STEPS), help="run this step in this process (what the parent starts)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: the median needs at least 20 calls")
    if a.step:
        res = train_step(a.reps, a.warmup) if a.step == "train" else grad_step(int(a.step[4:]), a.reps, a.warmup)
        print("RESULT " + json.dumps(res))
        return 0
    results = []
    for name in a.steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--warmup", str(a.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name])
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; stopping" % (name, STEPS[name]))
            return 1
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print("%s: exit status %d; stopping\n%s" % (name, r.returncode, (r.stdout + r.stderr)[-3000:]))
            return 1
        results.append(json.loads(line[-1][7:]))
        print(json.dumps(results[-1]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(notes(results, a.reps))
    return 0


if __name__ == "__main__":
    sys.exit(main())
