#!/usr/bin/env python3
"""mdd_ctc_variants at B = 64 utterances of T = 250 posterior frames, C = 45 classes, L = 64 canonical ids each, set against the only
way to get the same numbers without it: mdd_ctc_loss with no gradient over a batch whose targets are all the variants.

  variants        one mdd_ctc_variants call for the whole batch (substitutions, deletions and insertions), caller workspace
  variants_noins  the same without the insertion rows
  variants_wN     ``variants`` with N slots (waves) per workgroup instead of 4 (MDD_CTC_VARIANTS_WAVES)
  lattice_nll     mdd_ctc_loss without gradient on the canonical ids: the alpha scan alone, for scale
  brute_one       mdd_ctc_loss without gradient over the (2L+1)(C-1)-odd variants of ONE utterance (its posteriors repeated once per
                  variant: the batch of all 64 utterances' variants would take 16 GB of posteriors); the whole batch costs 64 of these

Each step runs in a child process of its own under a time limit (a step that fails or hangs ends the run; nothing is started after
it) and reports the mean of --reps launches between two HIP events after --warmup untimed ones.  The parent prints one JSON line and
--out writes the notes file.  MDD_LIB_PATH selects the library, so ``--only brute_one,lattice_nll`` also runs on a build that lacks
mdd_ctc_variants.

Usage:  python tools/time_ctc_variants.py [--B 64] [--T 250] [--C 45] [--L 64] [--reps 20] [--warmup 3] [--step_timeout 120] [--only a,b] [--out PATH]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("variants", "variants_noins", "variants_w1", "variants_w2", "variants_w8", "lattice_nll", "brute_one")


def inputs(a):
    """Peaked posteriors along each utterance's own canonical ids (segments of one class, blanks between them), a few ids mispronounced."""
    import numpy as np
    rs = np.random.default_rng(7)
    x = rs.standard_normal((a.T, a.B, a.C)).astype(np.float32)
    ids = rs.integers(1, a.C, size=(a.B, a.L)).astype(np.int32)
    seg = max(1, a.T // (2 * a.L + 1))
    for b in range(a.B):
        for i in range(a.L):
            said = int(ids[b, i]) if rs.random() > 0.1 else int(rs.integers(1, a.C))
            x[(2 * i + 1) * seg:(2 * i + 2) * seg, b, said] += 6.0
            x[(2 * i) * seg:(2 * i + 1) * seg, b, 0] += 6.0
    return x, ids


def variant_targets(y, Cn):
    """Every one-edit variant of y (blank 0) as padded int64 targets and their lengths: the canonical itself first."""
    import numpy as np
    y = [int(v) for v in y]
    tg = [y]
    for i in range(len(y)):
        tg.append(y[:i] + y[i + 1:])
        tg.extend(y[:i] + [k] + y[i + 1:] for k in range(1, Cn) if k != y[i])
    for g in range(len(y) + 1):
        tg.extend(y[:g] + [k] + y[g:] for k in range(1, Cn))
    out = np.zeros((len(tg), len(y) + 1), np.int64)
    for n, t in enumerate(tg):
        out[n, :len(t)] = t
    return out, np.array([len(t) for t in tg], np.int64)


def child(a):
    import numpy as np
    import torch
    from ctc_attention_mispronunciation_amd import _lib
    if a.step.startswith("variants_w"):
        os.environ["MDD_CTC_VARIANTS_WAVES"] = a.step[len("variants_w"):]
    if a.step.startswith("variants"):
        L = _lib.lib()
    else:       # mdd_ctc_loss alone, bound by hand: a library from before mdd_ctc_variants loads too
        L = C.CDLL(_lib.LIB_PATH)
        L.mdd_last_error.restype = C.c_char_p
        L.mdd_ctc_loss.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    st = _lib.current_stream_ptr()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    x, ids_h = inputs(a)
    lp = torch.log_softmax(torch.from_numpy(x).cuda(), dim=-1).contiguous()
    res = dict(step=a.step)
    if a.step.startswith("variants"):
        lens = torch.full((a.B,), a.T, dtype=torch.int32, device="cuda")
        ids = torch.from_numpy(ids_h).cuda()
        nids = torch.full((a.B,), a.L, dtype=torch.int32, device="cuda")
        base = torch.empty((a.B,), dtype=torch.float64, device="cuda")
        sub = torch.empty((a.B, a.L, a.C), dtype=torch.float64, device="cuda")
        ins = torch.empty((a.B, a.L + 1, a.C), dtype=torch.float64, device="cuda")
        status = torch.empty((a.B,), dtype=torch.int32, device="cuda")
        need = L.mdd_ctc_variants_workspace_bytes(a.T, a.B, a.C, a.L)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        res["workspace_bytes"] = int(need)

        def fn():
            _lib.check(L.mdd_ctc_variants(p(lp), a.T, a.B, a.C, p(lens), p(ids), a.L, p(nids), a.L, 0, p(base), p(sub),
                                          p(ins) if a.step != "variants_noins" else None, p(status), p(ws), ws.numel(), st))
    else:
        if a.step == "lattice_nll":
            tg, tl, logp = torch.from_numpy(ids_h.astype(np.int64)).cuda(), torch.full((a.B,), a.L, dtype=torch.int64, device="cuda"), lp
        else:
            tg_h, tl_h = variant_targets(ids_h[0], a.C)
            tg, tl = torch.from_numpy(tg_h).cuda(), torch.from_numpy(tl_h).cuda()
            logp = lp[:, :1, :].expand(a.T, tg.shape[0], a.C).contiguous()
            res["targets"] = int(tg.shape[0])
        n = tg.shape[0]
        il = torch.full((n,), a.T, dtype=torch.int64, device="cuda")
        nll = torch.empty((n,), dtype=torch.float32, device="cuda")

        def fn():
            rc = L.mdd_ctc_loss(p(logp), a.T, n, a.C, p(tg), tg.shape[1], p(il), p(tl), 0, p(nll), None, None, 0, st)
            assert rc == 0, L.mdd_last_error().decode()
    for _ in range(a.warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    e1.synchronize()
    res["ms"] = e0.elapsed_time(e1) / a.reps
    if a.step == "variants":
        res["all_ok"] = bool((status.cpu().numpy() == 0).all())
        res["finite_fraction"] = float(torch.isfinite(sub).double().mean())
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=250)
    ap.add_argument("--C", type=int, default=45)
    ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step_timeout", type=int, default=120)
    ap.add_argument("--step", default=None, choices=STEPS)
    ap.add_argument("--only", default=None, help="comma-separated subset of the steps")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        return child(a)
    steps = [s for s in STEPS if a.only is None or s in a.only.split(",")]
    res = dict(B=a.B, T=a.T, C=a.C, L=a.L, reps=a.reps, library=os.environ.get("MDD_LIB_PATH", "built tree"))
    for step in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [x for k in ("B", "T", "C", "L", "reps", "warmup")
                                                                             for x in ("--" + k, str(getattr(a, k)))]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print("step %s ran past %d s; stopping" % (step, a.step_timeout), file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("step %s failed (%d); stopping\n%s" % (step, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        res[step] = json.loads(r.stdout.strip().splitlines()[-1])
    if "brute_one" in res:
        res["brute_batch_ms"] = res["brute_one"]["ms"] * a.B
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("One-edit CTC variants at B = %d, T = %d, C = %d, L = %d (tools/time_ctc_variants.py), mean ms of %d launches\n"
                    % (a.B, a.T, a.C, a.L, a.reps))
            for step in steps:
                f.write("  %-15s %.4f ms\n" % (step, res[step]["ms"]))
            if "brute_one" in res:
                f.write("  brute force for the batch = %d x brute_one (%d targets each): %.2f ms\n" % (a.B, res["brute_one"]["targets"], res["brute_batch_ms"]))
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
