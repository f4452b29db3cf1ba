"""The CPU side of the gate-clear training cases (tests/gate_clear_cases.py): what makes the bound of tests/test_conv_train.py legitimate,
that the table reaches the kernel edges it names, and that the bound has teeth.  No GPU.

  * clear_gates touches the two conv BatchNorm biases only, by at most its window, and is deterministic; the float64 step is finite.
  * The condition: at both ReLU sites the smallest |y| of the float64 run is at least 16 times ATen fp32's own max |y32 - y64| on the same
    case, and no gate differs between the two.  With that, a correct fp32 evaluation decides every gate as float64 does, and the conv.*
    gradients are as well conditioned as the tensors outside the CNN.  (A case that misses it gets another seed or window, not another factor.)
  * Teeth: two index errors of the kind the direct conv1 kernels could make -- a lost 128-position tile of the weight gradient where a
    workgroup walks two tiles, a lost last column of one stride class of the input gradient -- move a conv.* gradient by at least 10 times
    the bound the GPU test applies to that tensor of that case.  The float64 step's dz1 and conv1 input are taken with autograd hooks."""
import functools
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gate_clear_cases as gcc
from tests import geometry_cases as gc

NAMES = list(gcc.CASES)
BN_BIAS = ("conv.0.batch_norm.bias", "conv.1.batch_norm.bias")


@functools.lru_cache(maxsize=None)
def _margin(name):
    _, (sd, x, _, masks, _, _, _) = gcc.case(name)
    return gcc.gate_margin(sd, x, masks, gcc.P_DROP)


@pytest.mark.parametrize("name", NAMES)
def test_clear_gates_changes_only_the_two_biases(name):
    c = gcc.CASES[name]
    geom, (sd, x, x1, masks, tg, il, tl) = gcc.case(name)
    B, T, L, Lt = c.shape
    assert B * T >= 64
    sd0, x0, x10, masks0, tg0, il0, tl0 = gc.train_case(geom, c.seed, B, T, L, Lt, gcc.P_DROP)
    for a, b in ((x, x0), (x1, x10), (tg, tg0), (il, il0), (tl, tl0)) + tuple(zip(masks, masks0)):
        np.testing.assert_array_equal(a, b)
    assert list(sd) == list(sd0)
    for k in sd:
        assert sd[k].dtype == sd0[k].dtype and sd[k].shape == sd0[k].shape, k
        if k in BN_BIAS:
            assert float(np.abs(sd[k].astype(np.float64) - sd0[k]).max()) <= c.window, k
        else:
            np.testing.assert_array_equal(sd[k], sd0[k], err_msg=k)
    again = gcc.clear_gates(sd0, x0, masks0, gcc.P_DROP, c.window)
    for k in BN_BIAS:
        np.testing.assert_array_equal(again[k], sd[k], err_msg=k)
    assert x1.max() == geom.emb_rows - 1


@pytest.mark.parametrize("name", NAMES)
def test_float64_step_is_finite(name):
    (logp, loss, grads, run), d_aten = gcc.reference(name)
    assert np.isfinite(logp).all() and np.isfinite(loss) and loss > 0
    for k, g in list(grads.items()) + list(run.items()):
        assert np.isfinite(g).all(), k
    assert all(np.isfinite(v) for v in d_aten.values())


@pytest.mark.parametrize("name", NAMES)
def test_gate_margin_is_16_times_aten_fp32s_error(name):
    m = _margin(name)
    print("gate margin %s: min |y| %.2e %.2e, ATen fp32 max |y32 - y64| %.2e %.2e, ratio %.0f %.0f, gates differing %d %d"
          % ((name,) + m.min_abs + m.aten_err + tuple(a / e for a, e in zip(m.min_abs, m.aten_err)) + m.flips))
    for site in (0, 1):
        assert m.aten_err[site] > 0
        assert m.min_abs[site] >= 16.0 * m.aten_err[site], (name, site, m)
        assert m.flips[site] == 0, (name, site, m)


@pytest.mark.parametrize("name", NAMES)
def test_draw_is_well_conditioned(name):
    """The 2e-5 bounds presuppose a draw that does not amplify rounding: one fp32 rounding of every parameter (relative 2^-24, in float64)
    moves no gradient by more than 2e-6 of scale, a tenth of the bound -- an fp32 step is many roundings deep.  A property of the inputs,
    measured on the reference alone; a case that misses it gets another seed (gate_clear_cases.py: "last_direct")."""
    moved = gcc.rounding_response(name)
    print("rounding response %s: %.2e" % (name, moved))
    assert moved <= 2e-6, (name, moved)


def test_aten_fp32_on_cleared_gates_is_rounding_level():
    """What the clearing buys, on the reference itself: with the gates agreed, ATen fp32's distance from float64 on the held conv tensors is
    of the order of its distance outside the CNN (measured 0.4 .. 1.5 times it, 5e-7 .. 3e-5), not the 1e-3 of one flipped gate."""
    for name in NAMES:
        d = gcc.reference(name)[1]
        conv = max(v for k, v in d.items() if gcc.held(k))
        outside = max(v for k, v in d.items() if not k.startswith("conv."))
        print("ATen fp32 vs float64 %s: conv.* %.2e, outside the CNN %.2e" % (name, conv, outside))
        assert conv <= 1e-4, (name, conv, outside)


def test_table_reaches_what_it_claims():
    geoms = {n: gc.geometry(gcc.CASES[n].geom) for n in NAMES}
    w1 = {g.w1 for g in geoms.values()}
    assert {127, 128, 129, 65, 3, 2} <= w1 and any(w % 2 for w in w1)
    for n, g in geoms.items():          # the even / odd rule of the right edge: W2 = W1 / 2 or (W1 + 1) / 2
        assert g.w2 == (g.w1 + 1) // 2, n
    # dgrad's row count per stride class, nj = (W1 - par + 1) / 2 (csrc/train_conv1.hip:99), at the edges of its two 32-row MFMA tiles
    nj = {n: tuple((g.w1 - par + 1) // 2 for par in (0, 1)) for n, g in geoms.items()}
    assert nj["last_direct"] == (64, 64) and nj["ragged"] == (64, 63) and nj["one_row_tile2"] == (33, 32) and nj["half_tile"] == (30, 30)
    assert nj["odd"] == (61, 60) and nj["ref"] == (61, 61)
    # the direct kernels run for 32 channels and W1 <= 128 without the switch (csrc/train.hip:266)
    direct = {n for n, g in geoms.items() if g.channels == 32 and g.w1 <= 128}
    assert "first_im2col" not in direct and "ch4" not in direct and {"last_direct", "ragged", "w2_feat3", "w3"} <= direct
    assert {g.feat for g in geoms.values() if g.w1 == 2} == {3, 4}
    tp = {n: gcc.CASES[n].shape[1] // 2 for n in NAMES}
    assert 1 in tp.values() and any(t % 2 and t > 1 for t in tp.values())
    assert any((c.shape[0] * c.shape[1]) % 4 for c in gcc.CASES.values())
    for n, c in gcc.CASES.items():
        assert c.shape[1] % 2 == 0 and (c.shape[3] == 1 or tp[n] >= 2 * c.shape[3]), n      # every CTC row feasible
    # more tiles than workgroups in the conv1 weight gradient (wgrad_tiles restates csrc/train_conv1.hip:238-246), on the direct path
    B, T, _, _ = gcc.CASES["gridstride"].shape
    tiles, groups = gcc.wgrad_tiles(B, T, geoms["gridstride"].w2)
    assert (tiles, groups) == (519, 512) and "gridstride" in direct
    for n in NAMES:
        if n != "gridstride":
            t, g = gcc.wgrad_tiles(gcc.CASES[n].shape[0], gcc.CASES[n].shape[1], geoms[n].w2)
            assert t == g, n
    runs = set(gcc.RUNS)
    assert {("ref", "f32", False), ("ref", "f32", True), ("ref", "f32x6", False)} <= runs
    assert all(mode in ("f32", "f32x6") for _, mode, _ in runs)
    assert len({gcc.run_id(*r) for r in runs}) == len(gcc.RUNS)


# ------------------------------------------------------------------------------------------------------------------------- teeth
@functools.lru_cache(maxsize=None)
def _conv1_taps(name):
    """conv1's input a0 (after site 0's ReLU and mask), dloss/da0 and dloss/dz1 of ref_port.train_step in float64, by autograd hooks on
    the step's second convolution."""
    from oracle import ref_port
    _, inputs = gcc.case(name)
    got, real = {}, F.conv2d

    def conv2d(a, w, *args, **kw):
        z = real(a, w, *args, **kw)
        if a.requires_grad:                                            # conv1: its input carries a gradient, conv0's (the features) does not
            got["a0"] = a.detach().clone()
            a.register_hook(lambda g: got.__setitem__("da0", g.detach().clone()))
            z.register_hook(lambda g: got.__setitem__("dz1", g.detach().clone()))
        return z
    with mock.patch.object(ref_port.F, "conv2d", conv2d):
        grads = ref_port.train_step(*inputs, gcc.P_DROP, dtype=torch.float64)[2]
    assert set(got) == {"a0", "da0", "dz1"}
    return got, grads


def test_teeth_lost_wgrad_tile():
    """gridstride: conv1's weight gradient without the last of its 519 tiles of 128 output positions (in the kernel's order: (b, t', w')
    flattened, channels last) -- one of the seven tiles that a workgroup walks second."""
    name = "gridstride"
    geom, _ = gcc.case(name)
    got, grads = _conv1_taps(name)
    key = "conv.1.conv.weight"
    shape = grads[key].shape

    def wgrad(dz1):
        return torch.nn.grad.conv2d_weight(got["a0"], shape, dz1, stride=(2, 2), padding=(1, 1)).numpy()
    full = wgrad(got["dz1"])
    assert gcc.scaled_distance(full, grads[key]) <= 1e-12            # the hooks took the tensors the step used
    B, C, Tp, W2 = got["dz1"].shape
    tiles, groups = gcc.wgrad_tiles(B, 2 * Tp, W2)
    assert tiles > groups
    pos = got["dz1"].permute(0, 2, 3, 1).reshape(B * Tp * W2, C).clone()
    pos[(tiles - 1) * 128:] = 0.0
    moved = gcc.scaled_distance(wgrad(pos.reshape(B, Tp, W2, C).permute(0, 3, 1, 2).contiguous()), full)
    print("teeth %s: a lost last tile moves %s by %.2e of scale; the bound is %.2e" % (name, key, moved, gcc.bound(name, key)))
    assert moved >= 10.0 * gcc.bound(name, key), (moved, gcc.bound(name, key))


@pytest.mark.parametrize("name", ["odd", "last_direct"])
@pytest.mark.parametrize("cls", range(4))
def test_teeth_lost_dgrad_column(name, cls):
    """odd, last_direct: dloss/da0 with the last column of one of dgrad's four stride classes zeroed (class c: input rows t = (c >> 1) mod 2,
    columns w = (c & 1) + 2 j; the last one is j = nj - 1), carried on through site 0 to conv0's and its BatchNorm's gradients."""
    geom, (sd, x, _, masks, _, _, _) = gcc.case(name)
    got, grads = _conv1_taps(name)
    keys = ("conv.0.conv.weight", "conv.0.batch_norm.weight", "conv.0.batch_norm.bias")
    par, row = cls & 1, cls >> 1
    col = par + 2 * ((geom.w1 - par + 1) // 2 - 1)
    assert col in (geom.w1 - 1, geom.w1 - 2) and col % 2 == par

    def site0_grads(da0):
        p = {k: torch.tensor(sd[k], dtype=torch.float64).requires_grad_(True) for k in keys}
        z = F.conv2d(torch.as_tensor(x, dtype=torch.float64).unsqueeze(1), p[keys[0]], torch.tensor(sd["conv.0.conv.bias"], dtype=torch.float64),
                     stride=(1, 2), padding=(1, 1))
        a0 = F.relu(F.batch_norm(z, None, None, p[keys[1]], p[keys[2]], training=True)) * (torch.as_tensor(masks[0], dtype=torch.float64) / (1.0 - gcc.P_DROP))
        a0.backward(da0)
        return {k: v.grad.numpy() for k, v in p.items()}
    full = site0_grads(got["da0"])
    for k in keys:
        assert gcc.scaled_distance(full[k], grads[k]) <= 1e-12, k
    cut = got["da0"].clone()
    assert float(cut[:, :, row::2, col].abs().max()) > 0
    cut[:, :, row::2, col] = 0.0
    lost = site0_grads(cut)
    ratio = max(gcc.scaled_distance(lost[k], full[k]) / gcc.bound(name, k) for k in keys)
    print("teeth %s class %d: column %d lost moves a conv.0 gradient by %.0f times its bound" % (name, cls, col, ratio))
    assert ratio >= 10.0, (name, cls, ratio)
