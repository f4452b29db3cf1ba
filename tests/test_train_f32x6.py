"""Training precision mode 2, "f32x6": the large contractions of the training step (input projections, dW_ih, the dW_hh products, dX)
as reference-width f32x6 GEMMs on the bf16 matrix cores -- mode plumbing, the operand forms through mdd_diag_gemm_ops (indexing with
exact integers, arithmetic against float64 beside ATen's fp32), and the whole step against the float64 restatement on mode 0's bounds."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests.helpers import record_margin
from tests.test_gpu_parity import _train_model, _cuda, synth

pytestmark = pytest.mark.gpu

MDD_ERR_ARG = -1
FORMS = [(0, 0), (0, 1), (1, 1), (1, 0)]            # (ta, tb): projections | dX | the weight gradients | (not used by the step)
M_, N_ = 200, 132                                    # one full 192 x 128 tile and a partial one on each axis
CASES = [(40, 1), (776, 1), (776, 3)]                # (K, splits): K = 40 pads to 64; 776 -> 25 K-tiles, in 3 chunks of 9 (27: the last partly padding)


def _lib():
    from ctc_attention_mispronunciation_amd import _lib as L
    return L.lib()


def _stored(op, t):
    """The operand op [rows, K] as the step stores it: [K, rows] when t, else as it is; 4 floats of slack behind each row, filled with
    a value that would show in the product if it were read."""
    m = np.ascontiguousarray(op.T if t else op)
    out = np.full((m.shape[0], m.shape[1] + 4), 1e6, dtype=np.float32)
    out[:, :m.shape[1]] = m
    return out


SENTINEL = -7.5


def _gemm_ops(mode, ta, tb, opA, opB, splits):
    """C [M, N + 4] from mdd_diag_gemm_ops, prefilled with the sentinel"""
    M, K = opA.shape
    N = opB.shape[0]
    A, B = _stored(opA, ta), _stored(opB, tb)
    Ad, Bd = _cuda(A), _cuda(B)
    Cd = torch.full((M, N + 4), SENTINEL, device="cuda")
    L = _lib()
    rc = L.mdd_diag_gemm_ops(mode, ta, tb, Ad.data_ptr(), A.shape[1], Bd.data_ptr(), B.shape[1], Cd.data_ptr(), N + 4, M, N, K, splits, None)
    assert rc == 0, L.mdd_last_error().decode()
    return Cd.cpu().numpy()


# ---------------------------------------------------------------------------- 2. operand forms, indexing exact
@pytest.mark.parametrize("K,splits", CASES)
@pytest.mark.parametrize("ta,tb", FORMS)
def test_operand_forms_integer_product_is_exact(ta, tb, K, splits):
    """Operands are integers in [-4, 4]: hi holds them whole, mid and lo are zero, every product (<= 16) and partial sum (<= 16 K) is
    an integer below 2^24, so any order of accumulation is exact and C must equal the integer product bit for bit.  A row, column,
    K-tile, chunk or plane taken from the wrong place shows as a wrong integer.  C is prefilled: every element inside M x N must be
    written, nothing in the four floats of slack behind column N."""
    rng = np.random.default_rng(1000 * K + 10 * splits + 2 * ta + tb)
    opA = rng.integers(-4, 5, (M_, K)).astype(np.float32)
    opB = rng.integers(-4, 5, (N_, K)).astype(np.float32)
    want = (opA.astype(np.int64) @ opB.astype(np.int64).T).astype(np.float32)
    got = _gemm_ops(3, ta, tb, opA, opB, splits)
    np.testing.assert_array_equal(got[:, N_:], np.full((M_, 4), SENTINEL, np.float32))
    np.testing.assert_array_equal(got[:, :N_], want)


def test_diag_entry_refuses_what_it_does_not_run():
    """an unknown mode and a result row shorter than N are MDD_ERR_ARG before any device work"""
    L = _lib()
    A, B, Cd = _cuda(np.zeros((256, 64), np.float32)), _cuda(np.zeros((128, 64), np.float32)), torch.zeros((256, 128), device="cuda")
    assert L.mdd_diag_gemm_ops(5, 0, 0, A.data_ptr(), 64, B.data_ptr(), 64, Cd.data_ptr(), 128, 256, 128, 64, 1, None) == MDD_ERR_ARG
    assert L.mdd_diag_gemm_ops(3, 0, 0, A.data_ptr(), 64, B.data_ptr(), 64, Cd.data_ptr(), 124, 256, 128, 64, 1, None) == MDD_ERR_ARG
    assert L.mdd_diag_gemm_ops(3, 0, 0, A.data_ptr(), 64, B.data_ptr(), 64, Cd.data_ptr(), 128, 256, 128, 64, 0, None) == MDD_ERR_ARG


# ---------------------------------------------------------------------------- 3. operand forms, arithmetic
@pytest.mark.parametrize("K,splits", CASES)
@pytest.mark.parametrize("ta,tb", FORMS)
def test_operand_forms_accuracy_beside_aten(ta, tb, K, splits):
    """Full 24-bit significands (operands as test_gemm_f32x6_accuracy draws them), |C - C64| / rms(C64) as a max and a mean, beside
    ATen's fp32 matmul on the CPU for the same operands (the reference's arithmetic).  K = 776: the condition the decode kernel
    meets, mean <= ATen's mean and max <= 1.5 x ATen's max.  K = 40: both sides are a couple of roundings and their ratio is noise,
    so max <= 4 x ATen's max (a lost or swapped mid / lo plane is 100x or more).  Mode 0 of the same entry checks the test: the exact
    kernel's result lies within the forward bound of an fp32 sum of K terms in any order, K u sum |a b| (u = 2^-24), of float64."""
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    rng = np.random.default_rng(7000 + 1000 * K + 10 * splits + 2 * ta + tb)
    opA = rng.standard_normal((M_, K)).astype(np.float32)
    opA[opA < 0] = 0.0
    opA[:, ::7] *= 30.0
    opB = (rng.uniform(-1, 1, (N_, K)) * 0.05).astype(np.float32)
    ref = opA.astype(np.float64) @ opB.astype(np.float64).T
    scale = float(np.sqrt((ref ** 2).mean()))
    aten = (torch.from_numpy(opA) @ torch.from_numpy(opB).T).numpy()
    x6 = _gemm_ops(3, ta, tb, opA, opB, splits)
    f32 = _gemm_ops(0, ta, tb, opA, opB, 1)
    for got in (x6, f32):
        np.testing.assert_array_equal(got[:, N_:], np.full((M_, 4), SENTINEL, np.float32))
    err = {k: (float(np.abs(v - ref).max()) / scale, float(np.abs(v - ref).mean()) / scale) for k, v in (("aten", aten), ("x6", x6[:, :N_]), ("f32", f32[:, :N_]))}
    tag = "train_f32x6_gemm_t%d%d_K%d_s%d_" % (ta, tb, K, splits)
    print(tag, "; ".join("%s max %.2e mean %.2e" % (k, v[0], v[1]) for k, v in err.items()))
    for k, v in err.items():
        record_margin(tag + k + "_max_rel", v[0])
        record_margin(tag + k + "_mean_rel", v[1])
    bound = 1.01 * K * 2.0 ** -24 * (np.abs(opA).astype(np.float64) @ np.abs(opB).astype(np.float64).T)
    assert (np.abs(f32[:, :N_] - ref) <= bound).all(), "mode 0 (the test's own check)"
    if K == 40:
        assert err["x6"][0] <= 4.0 * err["aten"][0], err
    else:
        assert err["x6"][1] <= err["aten"][1] and err["x6"][0] <= 1.5 * err["aten"][0], err


# ---------------------------------------------------------------------------- whole steps, computed once and shared
# Shapes at which the dispatch rule of gemm_big (csrc/train.hip: M, N >= 128, K >= 64, M N K >= 2^27) sends every gemm_big form of every
# BiLSTM layer through the f32x6 path -- the smallest product is a dW_hh, 4H x H x (rows - B): 3.3e8 and 2.5e8 >= 2^27 = 1.3e8 -- so the
# batch sizes the issue names need no adjustment.  [0]: 576 rows, T' = 24; dW_ih of layers 1-3 and every dW_hh run split-K in 2 chunks of 9
# K-tiles.  [1]: T' = 23, 1012 rows (no multiple of 16 or 32: the contraction of the weight gradients is padded, the last row tile of
# the projections partial), split-K in 3 chunks.
SHAPES = [(384, 24, 48, 6), (256, 44, 46, 5)]


@functools.lru_cache(maxsize=None)
def _case(si):
    from oracle import ref_port
    H, B, T, L = SHAPES[si]
    geom = synth.Geometry(**dict(synth.REFERENCE, hidden=H))
    case = synth.train_case(geom, 77, B, T, L, max(1, min(6, T // 4)))       # ragged lengths, given dropout masks
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    ref = ref_port.train_step(*case, 0.2, dtype=torch.float64)
    return geom, case, ref


def _step(si, mode, model=None):
    """One training step in `mode` on a fresh model (or on `model`): log-probs, loss, gradients, all on the CPU; and the model"""
    from ctc_attention_mispronunciation_amd.train import CTCLoss
    geom, (sd, x, x1, masks, tg, il, tl), _ = _case(si)
    if model is None:
        model = _train_model(geom, sd)
    model.train_precision = mode
    model._dropout_masks = [torch.from_numpy(m) for m in masks]
    model.zero_grad()
    out = model(_cuda(x), _cuda(x1))
    loss = CTCLoss(reduction="sum")(out, torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)) / SHAPES[si][1]
    loss.backward()
    grads = {k: p_.grad.detach().cpu().clone() for k, p_ in model.named_parameters()}
    return out.detach().cpu().clone(), float(loss.detach()), grads, model


@functools.lru_cache(maxsize=None)
def _fresh(si, mode):
    return _step(si, mode)[:3]


# ---------------------------------------------------------------------------- 1. mode plumbing
def test_mode_plumbing():
    """mdd_train_set_precision takes 0, 1 and 2 and refuses 3 and -1 with MDD_ERR_ARG, naming the three modes; a refused call leaves
    the mode as it was (the next forward gives mode 2's bits, which are not mode 0's); model.train_precision = "f32x6" reaches the
    handle; an unknown string is a ValueError that names the valid ones."""
    from ctc_attention_mispronunciation_amd.train import TrainHandle
    L = _lib()
    geom, (sd, x, x1, masks, _, _, _), _ = _case(0)
    model = _train_model(geom, sd)
    h = TrainHandle(model._config(), 0)
    for mode in (0, 1, 2):
        assert L.mdd_train_set_precision(h.handle, mode) == 0, L.mdd_last_error().decode()
    for mode in (3, -1):
        assert L.mdd_train_set_precision(h.handle, mode) == MDD_ERR_ARG
        msg = L.mdd_last_error().decode()
        assert "0" in msg and "1" in msg and "2" in msg and "f32x6" in msg, msg
    h.close()
    model.train_precision = "f32x6"
    model._dropout_masks = [torch.from_numpy(m) for m in masks]
    first = model(_cuda(x), _cuda(x1)).detach().cpu()
    assert model._train_handle.precision == "f32x6"
    assert torch.equal(first, _fresh(0, "f32x6")[0]) and not torch.equal(first, _fresh(0, "f32")[0])
    assert L.mdd_train_set_precision(model._train_handle.handle, 3) == MDD_ERR_ARG
    again = model(_cuda(x), _cuda(x1)).detach().cpu()
    assert torch.equal(again, first)
    model.train_precision = "fp8"
    with pytest.raises(ValueError, match="f32x6") as e:
        model(_cuda(x), _cuda(x1))
    assert "bf16x3" in str(e.value) and "'f32'" in str(e.value)


# ---------------------------------------------------------------------------- 4. whole step against float64
@pytest.mark.parametrize("si", [0, 1])
def test_step_meets_exact_mode_bounds_against_float64(si):
    """Mode f32x6 against oracle/ref_port.train_step in float64 on MODE 0's bounds of test_train_step_split_bf16_variant (the mode's claim
    is reference width): log-probs 1e-4, loss 1e-5 relative, every gradient outside the CNN within 2e-5 of its scale, conv.* 3e-3.
    Mode f32 runs beside it on the same case; both distances are recorded (train_f32x6_*)."""
    _, _, (logp, loss, grads, _) = _case(si)
    H, B, T, L = SHAPES[si]
    worst = {}
    for mode in ("f32", "f32x6"):
        out, l2, g = _fresh(si, mode)
        dl = float(np.abs(out.numpy() - logp).max())
        errs = sorted(((float(np.abs(g[k].numpy() - grads[k]).max()) / max(1.0, float(np.abs(grads[k]).max())), k)
                       for k in g if not k.endswith("conv.bias")), reverse=True)
        rnn = max(e for e, k in errs if not k.startswith("conv."))
        cnn = max(e for e, k in errs if k.startswith("conv."))
        print(mode, "H=%d B=%d T=%d: max |dlogp| %.2e, loss rel %.2e, grad err / scale outside the CNN %.2e, conv.* %.2e; largest %s"
              % (H, B, T, dl, abs(l2 - loss) / abs(loss), rnn, cnn, [(k, "%.1e" % e) for e, k in errs[:4]]))
        tag = "train_f32x6_H%d_B%d_%s_" % (H, B, mode)
        record_margin(tag + "logp_abs", dl, 1e-4)
        record_margin(tag + "loss_rel", abs(l2 - loss) / abs(loss), 1e-5)
        record_margin(tag + "grad_rel", rnn, 2e-5)
        record_margin(tag + "conv_grad_rel", cnn, 3e-3)
        worst[mode] = (dl, abs(l2 - loss) / abs(loss), errs)
    for mode in ("f32", "f32x6"):
        dl, lr, errs = worst[mode]
        assert dl <= 1e-4, (mode, dl)
        assert lr <= 1e-5, (mode, lr)
        for e, k in errs:
            assert e <= (3e-3 if k.startswith("conv.") else 2e-5), (mode, k, e)


# ---------------------------------------------------------------------------- 5. the path is taken
def test_mode_2_results_are_not_mode_0_bits():
    """A mode 2 that fell back to the exact kernels everywhere would pass the float64 test: the forward projection (log-probs), a dW
    (rnns.3 weight_ih) and layer 0's dX (which is all that reaches conv.1's weight gradient) must each differ bitwise from mode 0."""
    o0, _, g0 = _fresh(0, "f32")
    o2, _, g2 = _fresh(0, "f32x6")
    assert not torch.equal(o0, o2)
    for k in ("rnns.3.rnn.weight_ih_l0", "conv.1.conv.weight"):
        assert not torch.equal(g0[k], g2[k]), k


# ---------------------------------------------------------------------------- 6. determinism and mode isolation
@pytest.mark.parametrize("si", [0, 1])
def test_deterministic_and_modes_do_not_leak(si):
    """Two mode-2 steps on fresh models give bit-identical results (split-K partials summed in a fixed order, no atomics); a handle
    switched 2 -> 0 gives the bits of a handle that was never in mode 2 (no stale planes or partials reused)."""
    o_a, l_a, g_a = _fresh(si, "f32x6")
    o_b, l_b, g_b, model = _step(si, "f32x6")
    assert torch.equal(o_a, o_b) and l_a == l_b
    for k in g_a:
        assert torch.equal(g_a[k], g_b[k]), k
    o_c, l_c, g_c, _ = _step(si, "f32", model=model)
    o_0, l_0, g_0 = _fresh(si, "f32")
    assert torch.equal(o_c, o_0) and l_c == l_0
    for k in g_0:
        assert torch.equal(g_c[k], g_0[k]), k
