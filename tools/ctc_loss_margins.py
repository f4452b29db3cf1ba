#!/usr/bin/env python3
"""Measure mdd_ctc_loss against the float64 reference over every run of tests/ctc_loss_cases.py (``runs``: each case through the kernel it
is routed to, and every wave-form case again with the generic kernel forced), and beside each the error of ATen's fp32 run of the same
input.  tests/test_ctc_loss_forms.py asserts, per kernel form, the larger of the project's present bound and twice the worst figure here.
One process, one pass; prints one JSON line and writes it to --out (default profiles/ctc_loss_margins.json).

Usage:  python tools/ctc_loss_margins.py [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_loss_margins.json"))
    a = ap.parse_args()
    import torch
    from tests import ctc_loss_cases as cc
    from tests import test_ctc_loss_forms as tf
    runs, worst = {}, {}
    for name, form, forced in cc.runs():
        if forced:
            os.environ["MDD_CTC"] = "generic"
        else:
            os.environ.pop("MDD_CTC", None)
        c = cc.case(name)
        T, B, Cn = c.lp.shape
        err = tf.measure(name)[0]
        aten_nll, aten_grad = cc.aten_err(name)
        runs[cc.run_id(name, form, forced)] = dict(case=name, form=form, forced=forced, T=T, B=B, C=Cn, L=int(c.tg.shape[1]), blank=c.blank,
                                                   aten_nll_rel_err=aten_nll, aten_grad_abs_err=aten_grad, **err)
        w = worst.setdefault(form, dict(nll_rel_err=0.0, grad_abs_err=0.0))
        for k in w:
            w[k] = max(w[k], err[k])
    os.environ.pop("MDD_CTC", None)
    res = dict(runs=runs, worst=worst, bound_factor=cc.MARGIN_FACTOR, present_nll_rtol=cc.NLL_RTOL, present_grad_atol=cc.GRAD_ATOL,
               device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
               compute_units=torch.cuda.get_device_properties(0).multi_processor_count)
    print(json.dumps(res, sort_keys=True))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
