#!/usr/bin/env python3
"""mdd_ctc_confnet_best beside the forward sweep of mdd_ctc_confnet on the error network of the same canonical ids (2L + 1 slots,
error_prior 0.05), at the shapes tools/time_ctc_confnet.py uses -- B = 64 utterances of T = 250 posterior frames, C = 45 classes, L = 64
canonical ids, so J = 129 slots -- and at the single-word shape T = 25, L = 5 (J = 11).

  best           one mdd_ctc_confnet_best call with path and seg, caller workspace: max-product sweep, backpointer stores, backtrace
  best_bare      the same with path_dev = seg_dev = NULL (the backtrace still runs: reading needs it)
  best_sweep     best_bare on the same network with its last slot closed (no arc at all): no reading has a path, so the sweep and its
                 backpointer stores run in full and the backtrace does not -- best_bare minus this is what the backtrace costs
  confnet_total  one mdd_ctc_confnet call with post_dev = NULL: the sum-product forward sweep alone, from the same library

Each step runs in a child process of its own under a time limit (a step that fails or hangs ends the run; nothing is started after it)
and reports the mean of --reps launches between two HIP events after --warmup untimed ones.  The parent prints one JSON line and --out
writes the notes file (default profiles/ctc_confnet_best_notes.txt).

Usage:  python tools/time_ctc_confnet_best.py [--B 64] [--C 45] [--shapes 250x64,25x5] [--reps 10] [--warmup 2] [--step_timeout 120] [--out PATH]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("best", "best_bare", "best_sweep", "confnet_total")
PRIOR = 0.05


def child(a):
    import torch
    from ctc_attention_mispronunciation_amd import _lib
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import error_network
    from tools.time_ctc_variants import inputs
    L = _lib.lib()
    st = _lib.current_stream_ptr()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    x, ids_h = inputs(a)
    lp = torch.log_softmax(torch.from_numpy(x).cuda(), dim=-1).contiguous()
    lens = torch.full((a.B,), a.T, dtype=torch.int32, device="cuda")
    ids = torch.from_numpy(ids_h).cuda()
    nids = torch.full((a.B,), a.L, dtype=torch.int32, device="cuda")
    status = torch.empty((a.B,), dtype=torch.int32, device="cuda")
    w, nslots = error_network(ids, nids, a.C, 0, PRIOR)
    J = 2 * a.L + 1
    if a.step == "best_sweep":
        w[:, J - 1, :] = float("-inf")
    res = dict(step=a.step, slots=J)
    if a.step == "confnet_total":
        total = torch.empty((a.B,), dtype=torch.float64, device="cuda")
        need = L.mdd_ctc_confnet_workspace_bytes(a.T, a.B, a.C, J, 0)
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")

        def fn():
            _lib.check(L.mdd_ctc_confnet(p(lp), a.T, a.B, a.C, p(lens), p(w), J, p(nslots), J, 0, p(total), None, p(status), p(ws), ws.numel(), st))
    else:
        full = a.step == "best"
        score = torch.empty((a.B,), dtype=torch.float64, device="cuda")
        reading = torch.empty((a.B, J), dtype=torch.int32, device="cuda")
        path = torch.empty((a.B, a.T), dtype=torch.int32, device="cuda")
        seg = torch.empty((a.B, J, 2), dtype=torch.int32, device="cuda")
        need = L.mdd_ctc_confnet_best_workspace_bytes(a.T, a.B, a.C, J)
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")

        def fn():
            _lib.check(L.mdd_ctc_confnet_best(p(lp), a.T, a.B, a.C, p(lens), p(w), J, p(nslots), J, 0, p(score), p(reading), p(status),
                                              p(path) if full else None, p(seg) if full else None, p(ws), ws.numel(), st))
    res["workspace_bytes"] = int(need)
    for _ in range(a.warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    e1.synchronize()
    res["ms"] = e0.elapsed_time(e1) / a.reps
    res["all_ok"] = bool((status.cpu().numpy() == (1 if a.step == "best_sweep" else 0)).all())      # best_sweep: all infeasible
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--C", type=int, default=45)
    ap.add_argument("--shapes", default="250x64,25x5", help="comma-separated TxL pairs")
    ap.add_argument("--T", type=int, default=None)
    ap.add_argument("--L", type=int, default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step_timeout", type=int, default=120)
    ap.add_argument("--step", default=None, choices=STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_confnet_best_notes.txt"))
    a = ap.parse_args()
    if a.step:
        return child(a)
    res = dict(B=a.B, C=a.C, reps=a.reps, error_prior=PRIOR, shapes={})
    for shape in a.shapes.split(","):
        T, L = (int(v) for v in shape.split("x"))
        here = res["shapes"][shape] = dict(T=T, L=L, slots=2 * L + 1)
        for step in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--T", str(T), "--L", str(L)]
            cmd += [x for k in ("B", "C", "reps", "warmup") for x in ("--" + k, str(getattr(a, k)))]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                print("step %s at %s ran past %d s; stopping" % (step, shape, a.step_timeout), file=sys.stderr)
                return 1
            if r.returncode != 0:
                print("step %s at %s failed (%d); stopping\n%s" % (step, shape, r.returncode, r.stderr[-2000:]), file=sys.stderr)
                return 1
            here[step] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("Best reading of the error network beside the sum-product forward sweep (tools/time_ctc_confnet_best.py), B = %d, C = %d, "
                    "error_prior %.2f, mean ms of %d launches\n" % (a.B, a.C, PRIOR, a.reps))
            for shape, here in res["shapes"].items():
                f.write("T = %d, L = %d (J = %d slots)\n" % (here["T"], here["L"], here["slots"]))
                for step in STEPS:
                    f.write("  %-14s %10.4f ms   workspace %d bytes\n" % (step, here[step]["ms"], here[step]["workspace_bytes"]))
                f.write("  best / confnet_total = %.2f, backtrace (best_bare - best_sweep) = %.4f ms\n"
                        % (here["best"]["ms"] / here["confnet_total"]["ms"], here["best_bare"]["ms"] - here["best_sweep"]["ms"]))
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
