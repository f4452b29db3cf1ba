#!/usr/bin/env python3
"""Measure the CTC-only forward (mdd_create_ctc) against float64 over every case of tests/test_ctc_only.py -- every geometry of
tests/ctc_only_cases.py (both forms of ctc_tail) at R = 21, 561 and 1 rows, 1 and 6 layers at R = 561, in the three arithmetic modes --
and against the reference's own fp32 output (G15).  Per case and mode two figures: the log-probs against the float64 forward, and against
the float64 tail (BatchNorm + Linear + log-softmax) of the tapped fp32 output of the last BiLSTM layer, which is ctc_tail's own error.
The tests' bound is 1e-4 on both.  One process, one pass; prints one JSON line and writes it to --out (default
profiles/ctc_only_margins.json).

Usage:  python tools/ctc_only_margins.py [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_only_margins.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    from tests import ctc_only_cases as cc
    from tests import test_ctc_only as tc
    from tests.helpers import jload, npz
    cases, worst, worst_tail = {}, 0.0, 0.0
    todo = [(n, k, cc.SHAPES) for n, (k, _) in sorted(cc.CASES.items())] + [(n, k, cc.SHAPES[1:2]) for n, (k, _) in sorted(cc.LAYER_CASES.items())]
    for name, kwargs, shapes in todo:
        geom = cc.geometry(kwargs)
        res = tc.measure_case(name, kwargs, shapes=shapes)
        cases[name] = dict(tail_form=cc.tail_form(geom),
                           precision_in_effect={p: cc.expected_precision(geom, p) for p in tc.PRECISIONS},
                           max_abs_err={k: dict(forward_vs_float64=v[0], tail_vs_float64_of_tapped_last_layer=v[1]) for k, v in sorted(res.items())})
        worst = max([worst] + [v[0] for v in res.values()])
        worst_tail = max([worst_tail] + [v[1] for v in res.values()])
    meta, g = jload("g15_ctc_only.json"), npz("g15_ctc_only.npz")
    golden = {}
    for case in meta["cases"]:
        geom = synth.Geometry(ctc_only=True, **case["geom"])
        sd = synth.synth_state_dict(geom, seed=case["seed"])
        for p in tc.PRECISIONS:
            m = HipModel(geom, sd, precision=p)
            lp = m.forward(torch.from_numpy(g[case["tag"] + "_x"]).cuda(), None, sync_errors=True).cpu().numpy()
            golden["%s_%s" % (case["tag"], p)] = float(np.abs(lp - g[case["tag"] + "_logp"]).max())
            m.close()
    prop = torch.cuda.get_device_properties(0)
    res = dict(bound=cc.TOL, forward_max_abs_err=worst, tail_max_abs_err=worst_tail, g15_max_abs_err_vs_reference_fp32=golden, cases=cases,
               device=torch.cuda.get_device_name(0), arch=prop.gcnArchName, compute_units=prop.multi_processor_count)
    print(json.dumps(res, sort_keys=True))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
