#!/usr/bin/env python3
"""Measure the error of mdd_ctc_confnet against the float64 references over every case of tests/test_ctc_confnet.py (``all_cases``: the
enumeration of all readings on the tiny networks, the float64 lattice and its cut-row marginals on the rest) and, for the equalities
with mdd_ctc_variants, the gap between the two calls.  The test's bound is 4 x the first figure, capped at 1e-4.  One process, one pass;
prints one JSON line and writes it to --out (default profiles/ctc_confnet_margins.json).

Usage:  python tools/ctc_confnet_margins.py [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_confnet_margins.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from tests import test_ctc_confnet as tc
    from tests import test_ctc_variants as tv
    worst, count, sums, per_case = 0.0, 0, 0.0, {}
    for case in tc.all_cases():
        got, w, n = tc.run_case(case)
        s = 0.0
        for b in range(case["lp"].shape[1]):
            rows = got["post"][b, :int(case["nslots"][b])]
            if np.isfinite(got["total"][b]) and len(rows):
                s = max(s, float(np.abs(np.logaddexp.reduce(rows, axis=1) - got["total"][b]).max()))
        per_case[case["name"]] = dict(confnet_max_abs_err=w, finite_entries=n, slot_sum_max_abs_gap=s)
        worst, count, sums = max(worst, w), count + n, max(sums, s)
    case, y = tc.variants_case()
    got = tc.gpu_confnet(case["lp"], case["lens"], case["w"], case["nslots"], case["Jmax"], case["blank"])
    var = tv.gpu_variants(case["lp"], case["lens"], np.array([y] * 3, np.int32), np.array([len(y)] * 3, np.int32), len(y), case["blank"])
    gaps = dict(base=abs(float(got["total"][0] - var["base"][0])))
    for key, have, want in (("sub_row", got["post"][1, 5], var["sub"][1, 2]), ("ins_row", got["post"][2, 6], var["ins"][2, 3])):
        fin = np.isfinite(want)
        gaps[key] = float(np.abs(have[fin] - want[fin]).max())
    res = dict(confnet_max_abs_err=worst, finite_entries=count, slot_sum_max_abs_gap=sums, variants_max_abs_gap=gaps, bound_factor=4, bound_cap=1e-4,
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
