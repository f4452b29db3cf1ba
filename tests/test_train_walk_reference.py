"""The CPU side of the training walks (tests/train_walk_cases.py): what tests/test_train_walk.py, test_train_trajectory.py and test_adam.py
rest on, checked on the reference alone.

* every case's float64 loss is finite, every target fits its T' frames, B * T >= 64;
* each shape's note is true: gemm_big's rule, split_chunks, the two persistent limits and embed_bwd's chunk size of csrc/train.hip are
  restated below, every claim of NOTES is compared with them, every choice has a shape on each side, and every consecutive pair of the
  interleaved order changes at least one choice in every mode the geometry is walked in;
* adam_f64 is torch.optim.Adam on float64 CPU tensors to 1e-14 relative (six steps, an lr change, weight_decay 0 and 5e-4): exp_avg_sq
  element by element (without weight decay), the parameters and exp_avg relative to the tensor's largest magnitude -- ATen fuses the multiply-add of lerp_ and
  add(alpha=), numpy does not, and an element whose two terms cancel a hundredfold has 2e-14 of its own magnitude from that alone;
* the yardstick of tests/test_adam.py: torch.optim.Adam in fp32 on the CPU, on that test's inputs, against adam_f64.  The largest distance of
  exp_avg (of the tensor's scale) and of exp_avg_sq (relative) are committed as profiles/adam_margins.json; this test measures them again
  and holds them under twice the committed values (and writes the file where it is missing), so the yardstick cannot drift unnoticed."""
import json
import math
import os
import time

import numpy as np
import pytest
import torch

from tests import train_walk_cases as tw
from tests.helpers import ROOT, record_margin

MARGINS = os.path.join(ROOT, "profiles", "adam_margins.json")

# ---------------------------------------------------------------------------------------- csrc/train.hip's choices, restated
SPLIT_RULES = {     # tile_m, max_tiles, min_k, k_round, k_unit, wg_budget, max_chunks
    "exact": (128, 256, 1025, 1, 512, 512, 64),
    "x3": (128, 256, 2049, 1, 1024, 512, 16),
    "x6": (192, 256, 512, 32, 256, 256, 16),
}
PERSIST_FWD_MAX_B, PERSIST_BWD_MAX_B, EMBED_CHUNK = 512, 256, 1024


def split_chunks(arith, M, N, K):
    tile_m, max_tiles, min_k, k_round, k_unit, wg_budget, max_chunks = SPLIT_RULES[arith]
    tiles = -(-M // tile_m) * -(-N // 128)
    if tiles >= max_tiles or K < min_k:
        return 1
    return min(max_chunks, max(1, min(-(-K // k_round) * k_round // k_unit, wg_budget // tiles)))


def gemm_big(mode, M, N, K, ldc, may_split, k_major):
    """(kernel family, chunks) of one contraction C[M, N] over K."""
    macs = M * N * K
    if mode == "f32x6" and M >= 128 and N >= 128 and K >= 64 and macs >= 1 << 27:
        return "x6", split_chunks("x6", M, N, K) if may_split else 1
    if mode == "bf16x3" and M >= 256 and N >= 256 and K >= 256 and ldc % 4 == 0 and macs >= 1 << 30:
        return "x3", split_chunks("x3", M, N, K) if may_split else 1
    if may_split and k_major:
        return "exact", split_chunks("exact", M, N, K)
    return "exact", 1


def contractions(geom, shape):
    """name -> (M, N, K, ldc, may be cut, both operands [K, *]) of every gemm_big call of one step (bilstm_forward, lstm_backward)."""
    B, T, L = shape
    H, R, Rt = geom.hidden, (T // 2) * B, L * B
    G, G2 = 4 * H, 8 * H
    out = {}
    for tag, K, r, steps, bias in [(str(n), geom.rnn_in if n == 0 else 2 * H, R, T // 2, False) for n in range(geom.layers)] + [("t", geom.emb_dim, Rt, L, True)]:
        assert K % 4 == 0 and H % 4 == 0            # x6_ops_ok: every leading dimension a multiple of 4
        out["fwd" + tag] = (r, G2, K, G2, not bias, False)
        out["dwih" + tag] = (G2, K, r, K, True, True)
        if steps > 1:
            out["dwhh" + tag] = (G, H, r - B, H, True, True)
        out["dx" + tag] = (r, K, G2, K, True, False)
    return out


def choices(geom, shape, mode):
    """Everything the step's host code decides from the shape, as one comparable value."""
    B, T, L = shape
    persistent = mode == "bf16x3" and geom.hidden in (256, 384)
    fwd_tiles = 0 if not persistent or B > PERSIST_FWD_MAX_B else (1 if B <= 256 else 2)
    gemms = tuple(sorted((k, gemm_big(mode, *v)) for k, v in contractions(geom, shape).items()))
    return dict(gemms=gemms, persist=(fwd_tiles, persistent and B <= PERSIST_BWD_MAX_B), embed_chunks=-(-L * B // EMBED_CHUNK), tn1=(T // 2 == 1, L == 1))


def _names(geom, shape, mode, family, cut):
    return tuple(k for k, (fam, chunks) in choices(geom, shape, mode)["gemms"] if fam == family and (chunks > 1 or not cut))


ALL = [(n, s) for n in tw.GEOMS for s in tw.SHAPES[n]]
IDS = ["%s-B%d-T%d-L%d" % ((n,) + s) for n, s in ALL]


def test_tables_are_consistent():
    for name in tw.GEOMS:
        assert set(tw.NOTES[name]) == set(tw.SHAPES[name]) and len(set(tw.SHAPES[name])) == len(tw.SHAPES[name])
        orders = tw.walk_orders(name)
        assert len(orders) >= 3 and orders["mixed"][0] == orders["mixed"][-1]
        assert [tw.rows(s) for s in orders["up"]] == sorted(tw.rows(s) for s in tw.SHAPES[name])
        for o in orders.values():
            assert set(o) == set(tw.SHAPES[name])
        assert set(tw.TRAJECTORY[name]) <= set(tw.SHAPES[name])
        assert all(a != b for a, b in zip(tw.TRAJECTORY[name], tw.TRAJECTORY[name][1:]))        # the shape changes every step
        assert tw.EVAL_SHAPE not in tw.SHAPES[name]
    assert set(tw.MODES["H256_L1"]) == {"f32", "f32x6", "bf16x3"} and set(tw.MODES["feat120_H64_L2_C20"]) == {"f32", "bf16x3"}


@pytest.mark.parametrize("name,shape", ALL, ids=IDS)
def test_case_is_feasible_and_quick(name, shape):
    B, T, L = shape
    assert B * T >= 64 and T % 2 == 0
    t0 = time.perf_counter()
    geom, (sd, x, x1, masks, tg, il, tl), (logp, loss, grads, run) = tw.reference(name, shape)
    dt = time.perf_counter() - t0
    print("float64 step %s %s: %.2f s, loss %.4f" % (name, shape, dt, loss))
    assert math.isfinite(loss) and np.isfinite(logp).all() and logp.dtype == np.float64
    assert x.shape == (B, T, geom.feat) and x1.shape == (B, L) and x1.max() < geom.emb_rows
    assert (tl >= 1).all() and (tl <= il).all() and (il <= T // 2).all() and tg.shape[1] <= T // 2
    assert all(np.isfinite(g).all() for g in grads.values())
    assert len(masks) == 2 + geom.layers
    assert sd is tw.state_dict(name)                # the walk's weights never change


@pytest.mark.parametrize("name,shape", ALL, ids=IDS)
def test_note_is_true(name, shape):
    geom, note = tw.geometry(name), tw.NOTES[name][shape]
    got = choices(geom, shape, "f32")
    assert _names(geom, shape, "f32", "exact", True) == tuple(sorted(note["exact_split"])), (name, shape)
    assert got["embed_chunks"] == note["embed_chunks"] and got["tn1"] == note["tn1"], (name, shape, got)
    assert choices(geom, shape, "bf16x3")["persist"] == note["persist"], (name, shape)
    assert _names(geom, shape, "bf16x3", "x3", False) == tuple(sorted(note["x3"])), (name, shape)
    if name == "H256_L1":
        assert _names(geom, shape, "bf16x3", "x3", True) == tuple(sorted(note["x3_split"])), (name, shape)
        assert _names(geom, shape, "f32x6", "x6", False) == tuple(sorted(note["x6"])), (name, shape)
        assert _names(geom, shape, "f32x6", "x6", True) == tuple(sorted(note["x6_split"])), (name, shape)
    else:       # the variant's step must be mode 0's: same choices in both modes
        assert got == choices(geom, shape, "bf16x3"), (name, shape)


def test_every_choice_has_a_shape_on_each_side():
    def sides(name, f):
        return {bool(f(tw.NOTES[name][s])) for s in tw.SHAPES[name]}
    both = {True, False}
    for name in tw.GEOMS:
        assert sides(name, lambda n: n["exact_split"]) == both              # split_chunks, exact: K >= 1025
        assert sides(name, lambda n: n["embed_chunks"] > 1) == both         # embed_bwd_kernel's 1024-position chunks
        assert sides(name, lambda n: n["tn1"][0]) == both and sides(name, lambda n: n["tn1"][1]) == both
    h = "H256_L1"
    assert sides(h, lambda n: n["persist"][0] > 0) == both                  # persistent forward: B <= 512
    assert sides(h, lambda n: n["persist"][0] == 2) == both                 # its second tile: B > 256
    assert sides(h, lambda n: n["persist"][1]) == both                      # persistent BPTT: B <= 256
    for k in ("x6", "x6_split", "x3", "x3_split"):                          # gemm_big's two rules, split_chunks X6 (K >= 512) and X3 (K >= 2049)
        assert sides(h, lambda n: n[k]) == both, k
    # the same contraction on both sides of each K threshold, not merely some contraction
    for name, key, c in (("H256_L1", "exact_split", "dwhh0"), ("H256_L1", "exact_split", "dwiht"), ("H256_L1", "x3_split", "dwiht"),
                         ("H256_L1", "x6_split", "dwiht"), ("feat120_H64_L2_C20", "exact_split", "dwih0"), ("feat120_H64_L2_C20", "exact_split", "dwiht")):
        assert {c in tw.NOTES[name][s][key] for s in tw.SHAPES[name]} == both, (name, key, c)
    # K = 1025 and K = 1024 themselves
    g64 = tw.geometry("feat120_H64_L2_C20")
    assert contractions(g64, (41, 50, 25))["dwih0"][2] == 1025 and contractions(g64, (64, 32, 16))["dwih0"][2] == 1024


@pytest.mark.parametrize("name", tw.GEOMS)
def test_consecutive_shapes_change_a_choice(name):
    geom, order = tw.geometry(name), tw.walk_orders(name)["mixed"]
    for mode in tw.MODES[name]:
        for a, b in zip(order, order[1:]):
            assert choices(geom, a, mode) != choices(geom, b, mode), (name, mode, a, b)


# ---------------------------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_adam_f64_is_torch_adam_in_float64(wd):
    rng = np.random.Generator(np.random.PCG64(11))
    p0 = rng.standard_normal(777)
    pt = torch.nn.Parameter(torch.tensor(p0))
    opt = torch.optim.Adam([pt], lr=1e-3, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(777), np.zeros(777)
    for step in range(1, 7):
        lr = 1e-3 if step < 4 else 2.5e-4
        opt.param_groups[0]["lr"] = lr
        g = rng.standard_normal(777) * 10.0 ** rng.uniform(-6, 2, 777)
        pt.grad = torch.tensor(g)
        opt.step()
        p, m, v = tw.adam_f64(p, g, m, v, step, lr, wd=wd)
        st = opt.state[pt]
        assert int(st["step"]) == step
        if wd == 0:                 # a sum of non-negative terms: element by element (with weight decay g + wd p cancels as well)
            np.testing.assert_allclose(st["exp_avg_sq"].numpy(), v, rtol=1e-14, atol=0)
        for got, want in ((pt.detach(), p), (st["exp_avg"], m), (st["exp_avg_sq"], v)):     # of the tensor's scale: see the docstring
            assert float(np.abs(got.numpy() - want).max()) <= 1e-14 * float(np.abs(want).max())


def torch_adam_fp32(p, g, m, v, step, lr, wd):
    """One teacher-forced step of torch.optim.Adam in fp32 on the CPU from the given state; returns (p', m', v') as float32 arrays."""
    pt = torch.nn.Parameter(torch.tensor(np.array(p, dtype=np.float32)))
    opt = torch.optim.Adam([pt], lr=lr, weight_decay=wd)
    opt.state[pt] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.tensor(np.array(m, dtype=np.float32)),
                     "exp_avg_sq": torch.tensor(np.array(v, dtype=np.float32))}
    pt.grad = torch.tensor(np.array(g, dtype=np.float32))
    opt.step()
    st = opt.state[pt]
    assert int(st["step"]) == step
    return pt.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def test_adam_fp32_yardstick():
    e_m = e_v = 0.0
    for lr, wd in tw.ADAM_HYPER:
        for step, (p, g, m, v) in tw.adam_inputs(lr, wd).items():
            rp, rm, rv = tw.adam_f64(p, g, m, v, step, lr, wd=wd)
            tp, tm, tv = torch_adam_fp32(p, g, m, v, step, lr, wd)
            np.testing.assert_allclose(tp, rp, rtol=2e-6, atol=2e-7)        # the parameter bound of test_adam holds for the yardstick itself
            dm, dv = tw.adam_distances(tm, tv, rm, rv, p, g, m, v, wd)
            print("torch fp32 Adam lr %g wd %g step %d: exp_avg %.3e of scale, exp_avg_sq %.3e relative" % (lr, wd, step, dm, dv))
            e_m, e_v = max(e_m, dm), max(e_v, dv)
    measured = {"exp_avg_of_scale": e_m, "exp_avg_sq_relative": e_v}
    for k, val in measured.items():
        record_margin("adam_torch_fp32_" + k, val)
    if not os.path.exists(MARGINS):
        with open(MARGINS, "w") as f:
            json.dump(measured, f, indent=1, sort_keys=True)
    with open(MARGINS) as f:
        committed = json.load(f)
    for k, val in measured.items():
        assert 0 < val <= 2 * committed[k], (k, val, committed[k])
        assert committed[k] < 1e-5, k           # fp32 class: a handful of roundings of 6e-8, whatever the inputs
