"""The training step's CNN kernels at their index edges (GPU), on the gate-clear cases of tests/gate_clear_cases.py: odd and even conv
widths, W1 = 127 / 128 / 129 (the last widths of the direct conv1 kernels and the first of im2col), 65, 3 and 2, T' = 1 and 11, 66 rows,
519 weight-gradient tiles on 512 workgroups, 4 channels, and the shipped widths on both conv1 paths and in both reference-width modes.
Through the drop-in CTC_Model (tests/test_train_geometry.py's pattern) against oracle/ref_port.train_step in float64: log-probs, loss,
every parameter gradient and the running statistics.

Bounds: tests/test_train_geometry.py's for everything it bounds -- log-probs 1e-4, loss 1e-5 relative, gradients 2e-5 of scale outside
the CNN, conv.bias only small, running statistics 1e-5 -- and, what these cases are for, every conv.* weight and BatchNorm gradient at

    max(2e-5, 4 d_ATen) of scale          instead of the other training tests' 3e-3

d_ATen being the distance of ATen's fp32 run of ref_port.train_step from the float64 run on that tensor of that case, computed here on the
CPU once per case (6e-8 .. 3e-5; measured on the GPU: conv.* <= 3.0e-6 of scale, at most 0.14 of the bound).  The bound is legitimate because no ReLU gate of these inputs is near zero
(tests/test_conv_train_reference.py holds the margin to 16 times ATen fp32's error in the pre-activations), and it has teeth: a lost
weight-gradient tile or input-gradient column moves a conv gradient by 50 to 7000 times it (the same file).  Distances, their ratio to
d_ATen and the gate margins are recorded under "convtrain_"."""
import numpy as np
import pytest
import torch

from tests import gate_clear_cases as gcc
from tests.helpers import record_margin
from tests.test_train_geometry import _cuda, _train_model

pytestmark = pytest.mark.gpu
TOL = 1e-4
_steps = {}              # (case, mode, switch) -> what the GPU step returned, so that the path check below does not run "ref" again


def _step(name, mode, im2col, monkeypatch):
    """One step of the drop-in model on the GPU: (log-probs, loss, {key: gradient}, {key: running statistic}) as numpy."""
    from ctc_attention_mispronunciation_amd.train import CTCLoss
    if (name, mode, im2col) in _steps:
        return _steps[name, mode, im2col]
    B, T, L, _ = gcc.CASES[name].shape
    geom, (sd, x, x1, masks, tg, il, tl) = gcc.case(name)
    if im2col:
        monkeypatch.setenv("MDD_TRAIN_CONV1_IM2COL", "1")       # read when the training handle is created, by the first forward
    else:
        monkeypatch.delenv("MDD_TRAIN_CONV1_IM2COL", raising=False)
    model = _train_model(geom, sd)
    model.train_precision = mode
    model._dropout_masks = [torch.from_numpy(np.array(m, copy=True)) for m in masks]
    out = model(_cuda(x), _cuda(x1))
    assert out.shape == (T // 2, B, geom.num_class)
    l2 = CTCLoss(reduction="sum")(out, torch.from_numpy(np.array(tg)), torch.from_numpy(np.array(il)), torch.from_numpy(np.array(tl))) / B
    l2.backward()
    for k, p_ in model.named_parameters():
        assert p_.grad is not None, k
    _steps[name, mode, im2col] = (out.detach().cpu().numpy(), float(l2.detach()), {k: p_.grad.cpu().numpy() for k, p_ in model.named_parameters()},
                                  {k: b_.cpu().numpy() for k, b_ in model.named_buffers() if "running_" in k})
    return _steps[name, mode, im2col]


@pytest.mark.parametrize("name,mode,im2col", gcc.RUNS, ids=[gcc.run_id(*r) for r in gcc.RUNS])
def test_conv_train_step_against_float64(name, mode, im2col, monkeypatch):
    _, (sd, x, _, masks, _, _, _) = gcc.case(name)
    (logp, loss, grads, run), d_aten = gcc.reference(name)
    out, l2, got, buffers = _step(name, mode, im2col, monkeypatch)
    e_logp = float(np.abs(out.astype(np.float64) - logp).max())
    e_loss = abs(l2 - loss) / abs(loss)
    assert set(got) == set(grads), set(got) ^ set(grads)
    errs = sorted(((gcc.scaled_distance(got[k], grads[k]), k) for k in got if not k.endswith("conv.bias")), reverse=True)
    outside = [(e, k) for e, k in errs if not k.startswith("conv.")]
    conv = sorted(((e / gcc.bound(name, k), e, k) for e, k in errs if gcc.held(k)), reverse=True)
    assert len(conv) == 6
    _, e_conv, k_conv = conv[0]                                  # the conv tensor nearest its bound
    tag = "convtrain_" + gcc.run_id(name, mode, im2col).replace("-", "_")
    margin = gcc.gate_margin(sd, x, masks, gcc.P_DROP)
    print(tag, "logp %.2e loss(rel) %.2e; outside the CNN %.2e (%s);" % (e_logp, e_loss, outside[0][0], outside[0][1]),
          "conv.* err / scale [bound; d_ATen]:", ["%s %.2e [%.1e; %.1e]" % (k, e, gcc.bound(name, k), d_aten[k]) for _, e, k in conv])
    record_margin(tag + "_logp", e_logp, TOL)
    record_margin(tag + "_loss_rel", e_loss, 1e-5)
    record_margin(tag + "_grad_worst", outside[0][0], 2e-5)
    record_margin(tag + "_grad_conv_worst", e_conv, gcc.bound(name, k_conv))
    record_margin(tag + "_grad_conv_worst_over_aten", e_conv / d_aten[k_conv])
    for site in (0, 1):
        record_margin(tag + "_gate_margin_site%d" % site, margin.min_abs[site])
        record_margin(tag + "_gate_margin_site%d_over_aten_err" % site, margin.min_abs[site] / margin.aten_err[site])
    assert e_logp <= TOL, (tag, e_logp)
    assert e_loss <= 1e-5, (tag, e_loss)
    for k, g in got.items():
        assert np.isfinite(g).all(), k
        if k.endswith("conv.bias"):     # exactly zero in exact arithmetic (a bias in front of a batch-statistics BatchNorm): only smallness compares
            assert float(np.abs(g).max()) < 1e-3, (tag, k)
    for e, k in errs:
        assert e <= (gcc.bound(name, k) if k.startswith("conv.") else 2e-5), (tag, k, e, d_aten[k])
    assert set(buffers) == set(run), set(buffers) ^ set(run)
    for k, b_ in buffers.items():
        np.testing.assert_allclose(b_, run[k], rtol=0, atol=1e-5, err_msg=k)


def test_ref_case_ran_both_conv1_paths(monkeypatch):
    """The bound cannot tell the direct conv1 kernels from im2col + GEMM (both meet it), so the switch is read from the bits: the two f32
    runs of the "ref" case (held to the bound above; taken from there when the whole file runs) give conv.1.conv.weight gradients that
    differ."""
    assert ("ref", "f32", False) in gcc.RUNS and ("ref", "f32", True) in gcc.RUNS
    direct, im2col = (_step("ref", "f32", switch, monkeypatch)[2]["conv.1.conv.weight"] for switch in (False, True))
    assert direct.shape == im2col.shape
    assert not np.array_equal(direct, im2col)
