#!/usr/bin/env python3
"""CTC forced alignment (mdd_ctc_align) at the benchmark's decode shape, B = 64 utterances of T = 250 posterior frames, C = 45 classes,
about 40 ids each, set against two yardsticks on the same posteriors:

  align          mdd_ctc_align on the greedy ids, Lmax = T (what the decoders hand over: no host bound on nids, four labels per lane)
  align_bounded  the same with Lmax = 64 (a host that knows nids <= 64: two labels per lane)
  align_generic  the general kernel (MDD_CTC_ALIGN=generic), Lmax = T
  ctc_nll        mdd_ctc_loss without gradient on the same targets: the same lattice with fp64 log-adds
  greedy         mdd_greedy

Each step runs in a child process of its own under a time limit (a step that fails or hangs ends the run; nothing is started after
it) and reports the mean of --reps launches between two HIP events after --warmup untimed ones.  The parent prints one JSON line
with the five times and the wave form's LDS bytes, and --out writes the notes file.

Usage:  python tools/time_ctc_align.py [--B 64] [--T 250] [--C 45] [--ids 40] [--reps 50] [--warmup 5] [--step_timeout 120] [--out PATH]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = ("align", "align_bounded", "align_generic", "ctc_nll", "greedy")


def wave_lds_bytes(T, Cn, Lmax):
    """csrc/ctc_align.hip: log-probs + labels + path row + segment edges + backpointers (a nibble per label slot, >= a byte per lane)."""
    NL = 1 if Lmax <= 63 else (2 if Lmax <= 127 else 4)
    LC = 64 * NL
    return T * Cn * 4 + LC * 4 + T * 4 + 2 * LC * 4 + T * (64 if NL == 1 else 32 * NL)


def posteriors(a):
    """Peaked posteriors whose greedy decode has about a.ids ids per utterance: segments of one class, blanks between them."""
    import numpy as np
    rs = np.random.default_rng(7)
    x = rs.standard_normal((a.T, a.B, a.C)).astype(np.float32)
    seg = max(2, a.T // (2 * a.ids))
    for b in range(a.B):
        for k in range(a.T // seg):
            cls = 0 if k % 2 else int(rs.integers(1, a.C))
            x[k * seg:(k + 1) * seg, b, cls] += 6.0
    return x


def child(a):
    import torch
    from ctc_attention_mispronunciation_amd import _lib
    if a.step == "align_generic":
        os.environ["MDD_CTC_ALIGN"] = "generic"
    L = _lib.lib()
    st = _lib.current_stream_ptr()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    lp = torch.log_softmax(torch.from_numpy(posteriors(a)).cuda(), dim=-1).contiguous()
    lens = torch.full((a.B,), a.T, dtype=torch.int32, device="cuda")
    ids = torch.zeros((a.B, a.T), dtype=torch.int32, device="cuda")
    nids = torch.zeros((a.B,), dtype=torch.int32, device="cuda")
    _lib.check(L.mdd_greedy(p(lp), a.T, a.B, a.C, p(lens), 0, p(ids), p(nids), st))
    torch.cuda.synchronize()
    n = nids.cpu().numpy()
    Lmax = 64 if a.step == "align_bounded" else a.T
    assert int(n.max()) <= Lmax - 1, "the bounded run needs nids < Lmax"
    score = torch.empty((a.B,), dtype=torch.float32, device="cuda")
    status = torch.empty((a.B,), dtype=torch.int32, device="cuda")
    path = torch.empty((a.B, a.T), dtype=torch.int32, device="cuda")
    seg = torch.empty((a.B, a.T, 2), dtype=torch.int32, device="cuda")
    seg_logp = torch.empty((a.B, a.T), dtype=torch.float32, device="cuda")
    need = L.mdd_ctc_align_workspace_bytes(a.T, a.B, a.C, Lmax)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    tg, il, tl = ids.long(), lens.long(), nids.long()
    nll = torch.empty((a.B,), dtype=torch.float32, device="cuda")

    def align():
        _lib.check(L.mdd_ctc_align(p(lp), a.T, a.B, a.C, p(lens), p(ids), a.T, p(nids), Lmax, 0, p(score), p(status), p(path), p(seg),
                                   p(seg_logp), p(ws), ws.numel(), st))

    def ctc_nll():
        _lib.check(L.mdd_ctc_loss(p(lp), a.T, a.B, a.C, p(tg), a.T, p(il), p(tl), 0, p(nll), None, None, 0, st))

    def greedy():
        _lib.check(L.mdd_greedy(p(lp), a.T, a.B, a.C, p(lens), 0, p(ids), p(nids), st))

    fn = {"ctc_nll": ctc_nll, "greedy": greedy}.get(a.step, align)
    for _ in range(a.warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    e1.synchronize()
    res = dict(step=a.step, ms=e0.elapsed_time(e1) / a.reps, mean_ids=float(n.mean()), max_ids=int(n.max()), workspace_bytes=int(need))
    if fn is align:
        res["all_ok"] = bool((status.cpu().numpy() == 0).all())
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=250)
    ap.add_argument("--C", type=int, default=45)
    ap.add_argument("--ids", type=int, default=40)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step_timeout", type=int, default=120)
    ap.add_argument("--step", default=None, choices=STEPS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        return child(a)
    res = dict(B=a.B, T=a.T, C=a.C, reps=a.reps, lds_bytes_Lmax_T=wave_lds_bytes(a.T, a.C, a.T), lds_bytes_Lmax_64=wave_lds_bytes(a.T, a.C, 64))
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + [x for k in ("B", "T", "C", "ids", "reps", "warmup")
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
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("CTC forced alignment at the decode shape (tools/time_ctc_align.py), mean ms of %d launches\n" % a.reps)
            for step in STEPS:
                f.write("  %-14s %.4f ms\n" % (step, res[step]["ms"]))
            f.write("  wave-form LDS bytes: %d at Lmax = T, %d at Lmax = 64\n" % (res["lds_bytes_Lmax_T"], res["lds_bytes_Lmax_64"]))
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
