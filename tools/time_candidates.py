#!/usr/bin/env python3
"""mdd_forward_candidates beside the two ways there were to get K conditioned posteriors before it, at T = 500 stacked frames, L = 40
canonical phonemes, H = 384, the default mode (f32x6):

    (B, K) = (1, 4), (8, 8), (64, 4), (128, 8)

Per shape, each figure the median of --reps single calls timed between two HIP events after --warmup untimed ones (graph replays):

    candidates_ms        forward_candidates(x, x1 [K,B,L])
    k_forwards_ms        K calls of forward(x, x1[k]) between one pair of events
    repeated_fused_ms    forward_fused on x repeated K times (K B rows through every stage)
    parent_k_forwards_ms the same K calls of forward through a built checkout of the commit before the feature (--parent-tree: its package
                         and its library), measured by a child process of this run, so on the same card in the same session
    expected_ratio       (28 + 1.6 K) / (30 K): the stage table's guess for candidates_ms / k_forwards_ms at B = 512-class shapes
    k1_*                 K = 1: forward_candidates against forward, five repeats of each median; the new entry must not be slower than
                         forward beyond the spread of forward's own five

Prints one JSON line per shape and, with --out, writes the notes file.

Usage:  python tools/time_candidates.py [--reps 20] [--warmup 5] [--parent-tree DIR] [--out profiles/candidates_notes.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("TIME_CANDIDATES_TREE") or ROOT)     # (the child of --parent-tree imports that tree's package)
SHAPES = ((1, 4), (8, 8), (64, 4), (128, 8))
T, L, H = 500, 40, 384


def median_ms(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    vals = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        vals.append(e0.elapsed_time(e1))
    return statistics.median(vals)


def inputs(geom, B, K):
    import numpy as np
    import torch
    from ctc_attention_mispronunciation_amd import synth
    x = torch.from_numpy(synth.synth_batch(geom, B=B, T=T, L=L, seed=5, ragged=False)[0]).cuda()
    rng = np.random.Generator(np.random.PCG64(7))
    x1 = torch.from_numpy(rng.integers(2, geom.emb_rows, size=(K, B, L)).astype(np.int64)).cuda()
    return x, x1


def measure(forward_only, reps, warmup):
    import torch
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    geom = synth.Geometry(**synth.REFERENCE)
    assert geom.hidden == H
    m = HipModel(geom, synth.synth_state_dict(geom, seed=1234))
    results = []
    for B, K in SHAPES:
        x, x1 = inputs(geom, B, K)
        Tp, C = T // 2, geom.num_class
        outs = [torch.empty((Tp, B, C), dtype=torch.float32, device="cuda") for _ in range(K)]

        def k_forwards():
            for k in range(K):
                m.forward(x, x1[k], out=outs[k])
        res = dict(B=B, K=K, T=T, L=L, H=H, mode=m.precision, k_forwards_ms=median_ms(k_forwards, reps, warmup))
        if not forward_only:
            out_c = torch.empty((K, Tp, B, C), dtype=torch.float32, device="cuda")
            xr, x1r = x.repeat(K, 1, 1), x1.reshape(K * B, L)
            frames = torch.full((K * B,), Tp, dtype=torch.int32, device="cuda")
            canon = torch.full((K * B,), L, dtype=torch.int32, device="cuda")
            out_f = torch.empty((Tp, K * B, C), dtype=torch.float32, device="cuda")
            res["candidates_ms"] = median_ms(lambda: m.forward_candidates(x, x1, out=out_c), reps, warmup)
            res["repeated_fused_ms"] = median_ms(lambda: m.forward_fused(xr, x1r, frames, canon, out=out_f), reps, warmup)
            torch.cuda.synchronize()
            same = all(torch.equal(out_c[k], outs[k]) for k in range(K))
            res["equals_k_forwards_bitwise"] = bool(same)
            res["candidates_over_k_forwards"] = res["candidates_ms"] / res["k_forwards_ms"]
            res["expected_ratio"] = (28 + 1.6 * K) / (30.0 * K)
            one = x1[:1].contiguous()
            out_1 = torch.empty((1, Tp, B, C), dtype=torch.float32, device="cuda")
            f5, c5 = [], []
            for _ in range(5):      # alternating: a drift of the card's clock falls on both
                f5.append(median_ms(lambda: m.forward(x, one[0], out=outs[0]), reps, warmup))
                c5.append(median_ms(lambda: m.forward_candidates(x, one, out=out_1), reps, warmup))
            res.update(k1_forward_ms=f5, k1_candidates_ms=c5,
                       k1_holds=statistics.median(c5) <= statistics.median(f5) + (max(f5) - min(f5)))
        results.append(res)
        del x, x1
    m.close()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the commit before the feature: K forwards through it, in a child process")
    ap.add_argument("--forward-only", action="store_true", help="(the child's mode) K forwards alone, one JSON list on stdout")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_candidates: no GPU; a time is measured on the MI355X or not at all")
    if a.forward_only:
        print(json.dumps(measure(True, a.reps, a.warmup)))
        return 0
    results = measure(False, a.reps, a.warmup)
    if a.parent_tree:
        env = dict(os.environ, TIME_CANDIDATES_TREE=os.path.abspath(a.parent_tree))
        env.pop("MDD_LIB_PATH", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--forward-only", "--reps", str(a.reps), "--warmup", str(a.warmup)],
                           env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit("time_candidates: the child of --parent-tree failed:\n" + r.stderr[-2000:])
        for res, par in zip(results, json.loads(r.stdout.strip().splitlines()[-1])):
            assert (res["B"], res["K"]) == (par["B"], par["K"])
            res["parent_k_forwards_ms"] = par["k_forwards_ms"]
            res["candidates_over_parent_k_forwards"] = res["candidates_ms"] / par["k_forwards_ms"]
    lines = []
    for res in results:
        res.update(device=torch.cuda.get_device_name(0), compute_units=torch.cuda.get_device_properties(0).multi_processor_count)
        lines.append(json.dumps(res, sort_keys=True))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("tools/time_candidates.py --reps %d --warmup %d%s: one JSON line per shape (see the tool's docstring for the fields)\n"
                    % (a.reps, a.warmup, " --parent-tree <the parent commit, built>" if a.parent_tree else ""))
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
