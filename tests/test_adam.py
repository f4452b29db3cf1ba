"""mdd_adam_step (adam_multi_kernel, csrc/train_rows.hip) against float64 Adam (GPU), through the C ABI with pointer arrays so that NULL entries
are possible, and once through train.Adam.  Cases of tests/train_walk_cases.py:

* n = 1, 47, 48, 49, 96, 97 tensors (the 48-entry kernel-argument table exactly full, one past it, two tables, one past that), sizes cycling
  through 1, 3, 255, 256, 1023, 1024, 1025, 4097 (both sides of the 1024-element chunk and of the 256-thread stride);
* skipped entries -- a NULL gradient, numel = 0 -- at the start of a table, at its 48th slot and as the whole tail (launch_adam_multi's
  `continue` and its `count == 0` break): they keep their bits;
* p, g, m, v of every tensor carved out of ONE allocation with 64 guard elements on each side: no guard changes, g is bit-identical afterwards;
* steps 1, 2, 10 and 1000 (fp32's 1 - 0.9^1000 is 1), (lr, weight_decay) = (1e-3, 5e-4) and (5e-4, 0), moments carried from a float64
  trajectory; one tensor with g = m = v = 0 (0 / (0 + eps): unchanged without weight decay, never NaN), one with |g| over 1e-12 .. 1e3.

Bounds against adam_f64, teacher-forced per step: parameters rtol 2e-6 / atol 2e-7 (test_adam_matches_torch_optim_adam's); exp_avg of the
tensor's scale and exp_avg_sq relative FOUR TIMES what torch.optim.Adam in fp32 on the CPU is away from float64 on the same inputs
(profiles/adam_margins.json, measured by tests/test_train_walk_reference.py: 1.2e-7 and 3.3e-7) -- the factor covers another equally valid
rounding sequence of the two to four fp32 operations per element (fused multiply-adds against ATen's separate mul_ / addcmul_ / lerp_).

Finding (profiles/train_walk_margins.json, "adam_*"): with beta2 passed as the float 0.999f the kernel formed 1.f - b2 = 0.0009999871,
-1.29e-5 relative, where torch rounds the double 1 - beta2 to 0.001f, and exp_avg_sq missed its bound (measured figures: DESIGN.md section 2).
mdd_adam_step now takes the betas as doubles and the host forms 1 - b, 1 - b^step and sqrt(1 - b2^step) in double, one float each."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import train_walk_cases as tw
from tests.helpers import ROOT, record_margin

pytestmark = pytest.mark.gpu
GUARD = 64
SENTINEL = np.float32(-777.25)
FACTOR = 4.0


def _bounds():
    with open(os.path.join(ROOT, "profiles", "adam_margins.json")) as f:
        m = json.load(f)
    return FACTOR * m["exp_avg_of_scale"], FACTOR * m["exp_avg_sq_relative"]


def _skips(n, pattern):
    """{index: "nograd" | "empty"} of the entries the launcher must pass over."""
    if pattern == "none":
        return {}
    if pattern == "edges":      # the first two entries of the first table, the 48th entry and the one after it
        return {i: k for i, k in ((0, "nograd"), (1, "empty"), (47, "nograd"), (48, "empty")) if i < n}
    assert pattern == "tail" and n > 48     # 48 live entries fill one table; everything after is skipped, so the next table stays empty
    return {i: ("nograd" if i % 2 else "empty") for i in range(48, n)}


def _layout(n):
    """Element offsets [i][k] (k = 0..3: p, g, m, v) of each tensor's payload in one flat buffer, and the buffer's length."""
    off, pos = [], 0
    for i in range(n):
        size = tw.ADAM_SIZES[i % len(tw.ADAM_SIZES)]
        row = []
        for _ in range(4):
            row.append(pos + GUARD)
            pos += size + 2 * GUARD
        off.append(row)
    return off, pos


def _run(n, pattern, step, lr, wd):
    from ctypes import c_int64, c_void_p
    from ctc_attention_mispronunciation_amd import _lib
    L = _lib.lib()
    p, g, m, v = (a[:tw.adam_offsets(n)[-1]] for a in tw.adam_inputs(lr, wd)[step])
    src = tw.adam_offsets(n)
    off, total = _layout(n)
    host = np.full(total, SENTINEL, dtype=np.float32)
    for i in range(n):
        for k, a in enumerate((p, g, m, v)):
            host[off[i][k]:off[i][k] + src[i + 1] - src[i]] = a[src[i]:src[i + 1]]
    dev = torch.from_numpy(host.copy()).cuda()
    base = dev.data_ptr()
    skips = _skips(n, pattern)
    arrs = [(c_void_p * n)() for _ in range(4)]
    for i in range(n):
        for k in range(4):
            arrs[k][i] = None if (k == 1 and skips.get(i) == "nograd") else base + 4 * off[i][k]
    numel = (c_int64 * n)(*[0 if skips.get(i) == "empty" else src[i + 1] - src[i] for i in range(n)])
    with torch.cuda.device(dev.device):
        _lib.check(L.mdd_adam_step(arrs[0], arrs[1], arrs[2], arrs[3], numel, n, step, C.c_float(lr), C.c_double(tw.BETAS[0]), C.c_double(tw.BETAS[1]),
                                   C.c_float(tw.EPS), C.c_float(wd), _lib.current_stream_ptr()))
        torch.cuda.synchronize()
    out = dev.cpu().numpy()
    # guards, the gradients and every skipped tensor: bit for bit
    keep = np.ones(total, dtype=bool)
    for i in range(n):
        if i in skips:
            continue
        for k in (0, 2, 3):
            keep[off[i][k]:off[i][k] + src[i + 1] - src[i]] = False
    changed = np.nonzero(out.view(np.int32)[keep] != host.view(np.int32)[keep])[0]
    assert changed.size == 0, ("guard, gradient or skipped element changed", n, pattern, step, np.nonzero(keep)[0][changed[:8]])
    got = [np.concatenate([out[off[i][k]:off[i][k] + src[i + 1] - src[i]] for i in range(n)]) for k in range(4)]
    live = [i for i in range(n) if i not in skips]
    return (p, g, m, v), got, live


CASES = [(n, pat) for n in tw.ADAM_COUNTS for pat in ("none", "edges")] + [(n, "tail") for n in (49, 96, 97)]


@pytest.mark.parametrize("n,pattern", CASES, ids=["n%d-%s" % c for c in CASES])
def test_adam_step_against_float64(n, pattern):
    tol_m, tol_v = _bounds()
    src = tw.adam_offsets(n)
    worst = [0.0, 0.0, 0.0]
    fails = []
    for lr, wd in tw.ADAM_HYPER:
        for step in tw.ADAM_STEPS:
            (p, g, m, v), (gp, gg, gm, gv), live = _run(n, pattern, step, lr, wd)
            assert np.isfinite(gp).all() and np.isfinite(gm).all() and np.isfinite(gv).all(), (n, pattern, step)
            rp, rm, rv = tw.adam_f64(p, g, m, v, step, lr, wd=wd)
            e_m, e_v = tw.adam_distances(gm, gv, rm, rv, p, g, m, v, wd, n=n, live=live)
            e_p = 0.0
            for i in live:
                s = slice(src[i], src[i + 1])
                e_p = max(e_p, float((np.abs(gp[s].astype(np.float64) - rp[s]) / (2e-7 + 2e-6 * np.abs(rp[s]))).max()))     # <= 1: inside rtol 2e-6, atol 2e-7
            if tw.ADAM_ZERO in live and wd == 0:            # 0 / (0 + eps): nothing moves
                z = slice(src[tw.ADAM_ZERO], src[tw.ADAM_ZERO + 1])
                assert np.array_equal(gp[z], p[z]) and not gm[z].any() and not gv[z].any(), (n, pattern, step)
            print("adam n %d %s lr %g wd %g step %4d: p %.3f of its bound, exp_avg %.3e of scale, exp_avg_sq %.3e relative" % (n, pattern, lr, wd, step, e_p, e_m, e_v))
            worst = [max(a, b) for a, b in zip(worst, (e_p, e_m, e_v))]
            if e_p > 1 or e_m > tol_m or e_v > tol_v:
                fails.append((lr, wd, step, e_p, e_m, e_v))
    tag = "adam_n%d_%s" % (n, pattern)
    record_margin(tag + "_param_of_bound", worst[0], 1.0)
    record_margin(tag + "_exp_avg_of_scale", worst[1], tol_m)
    record_margin(tag + "_exp_avg_sq_rel", worst[2], tol_v)
    assert not fails, (tag, "bounds: p 1, exp_avg %.2e, exp_avg_sq %.2e" % (tol_m, tol_v), fails)


def test_adam_class_against_float64():
    """The same update through train.Adam over a five-layer model's worth of parameters (53 tensors: the second launch of the table),
    three steps with an lr change: parameters, both moments and the step count, teacher-forced per step."""
    from ctc_attention_mispronunciation_amd.train import Adam
    tol_m, tol_v = _bounds()
    n = 53
    src = tw.adam_offsets(n)
    lr, wd = tw.ADAM_HYPER[0]
    p0, _, _, _ = tw.adam_inputs(lr, wd)[1]
    params = [torch.nn.Parameter(torch.from_numpy(p0[src[i]:src[i + 1]].copy()).cuda()) for i in range(n)]
    opt = Adam(params, lr=lr, weight_decay=wd)
    worst = [0.0, 0.0, 0.0]
    for step in (1, 2, 3):
        if step == 3:
            opt.param_groups[0]["lr"] = lr = 2.5e-4
        g = tw.adam_inputs(*tw.ADAM_HYPER[0])[(1, 2, 10)[step - 1]][1][:src[n]]
        before = []
        for i, q in enumerate(params):
            q.grad = torch.from_numpy(g[src[i]:src[i + 1]].copy()).cuda()
            st = opt.state.get(q, {})
            before.append((q.detach().cpu().numpy(), st["exp_avg"].cpu().numpy() if st else np.zeros(q.numel(), np.float32),
                           st["exp_avg_sq"].cpu().numpy() if st else np.zeros(q.numel(), np.float32)))
        opt.step()
        torch.cuda.synchronize()
        pb, mb, vb = (np.concatenate([b[k] for b in before]) for k in range(3))
        rp, rm, rv = tw.adam_f64(pb, g, mb, vb, step, lr, wd=wd)
        gp = np.concatenate([q.detach().cpu().numpy() for q in params])
        gm = np.concatenate([opt.state[q]["exp_avg"].cpu().numpy() for q in params])
        gv = np.concatenate([opt.state[q]["exp_avg_sq"].cpu().numpy() for q in params])
        assert all(int(opt.state[q]["step"]) == step for q in params)
        e_m, e_v = tw.adam_distances(gm, gv, rm, rv, pb, g, mb, vb, wd, n=n)
        e_p = float((np.abs(gp.astype(np.float64) - rp) / (2e-7 + 2e-6 * np.abs(rp))).max())
        print("train.Adam step %d: p %.3f of its bound, exp_avg %.3e of scale, exp_avg_sq %.3e relative" % (step, e_p, e_m, e_v))
        worst = [max(a, b) for a, b in zip(worst, (e_p, e_m, e_v))]
    record_margin("adam_class_param_of_bound", worst[0], 1.0)
    record_margin("adam_class_exp_avg_of_scale", worst[1], tol_m)
    record_margin("adam_class_exp_avg_sq_rel", worst[2], tol_v)
    assert worst[0] <= 1 and worst[1] <= tol_m and worst[2] <= tol_v, worst
