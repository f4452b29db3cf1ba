#!/usr/bin/env python3
"""Measure the error of mdd_ctc_variants against the float64 brute force over every case of tests/test_ctc_variants.py (``all_cases``),
and beside it the error of mdd_ctc_loss's nll of the canonical ids on the same inputs.  The test's bound is 4 x the first figure, capped
at 1e-4.  One process, one pass; prints one JSON line and writes it to --out (default profiles/ctc_variants_margins.json).

Usage:  python tools/ctc_variants_margins.py [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_variants_margins.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from ctc_attention_mispronunciation_amd.hip_model import ctc_loss
    from tests import test_ctc_variants as tv
    worst, count, nll_worst, per_case = 0.0, 0, 0.0, {}
    for case in tv.all_cases():
        got, w, n = tv.run_case(case)
        lp, lens, ids, nids, blank = case["lp"], case["lens"], case["ids"], case["nids"], case["blank"]
        T, B, Cn = lp.shape
        stride = max(ids.shape[1], 1)
        tg = np.full((B, stride), (blank + 1) % Cn, np.int64)
        tg[:, :ids.shape[1]] = ids
        nll, _ = ctc_loss(torch.from_numpy(np.nan_to_num(lp, nan=0.0)).cuda(), torch.from_numpy(tg), torch.tensor(lens), torch.from_numpy(nids.astype(np.int64)),
                          blank=blank, want_grad=False)
        nll = nll.cpu().numpy().astype(np.float64)
        e = 0.0
        for b in range(B):
            Tb, L = min(max(int(lens[b]), 0), T), int(nids[b])
            ref = tv.brute(lp[:, b, :], Tb, [[int(v) for v in ids[b, :L]]], blank)[0]
            if np.isfinite(ref):
                e = max(e, abs(-nll[b] - ref))
        per_case[case["name"]] = dict(variants_max_abs_err=w, finite_entries=n, ctc_loss_nll_max_abs_err=e)
        worst, count, nll_worst = max(worst, w), count + n, max(nll_worst, e)
    res = dict(variants_max_abs_err=worst, finite_entries=count, ctc_loss_nll_max_abs_err=nll_worst, bound_factor=4, bound_cap=1e-4,
               bound=min(4 * worst, 1e-4), device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
               compute_units=torch.cuda.get_device_properties(0).multi_processor_count, cases=per_case)
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
