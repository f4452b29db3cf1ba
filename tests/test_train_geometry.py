"""The training step across the plan space (GPU): the geometries of tests/geometry_cases.py::TRAIN -- lstm_step_kernel<1> and
lstm_bwd_step_kernel<0> on full 16-unit tiles (H 64) and on a ragged one (H 20, 4 channels), direct conv1 at W1 = 60, conv1 through im2col
by its real trigger W1 > 128, 1 and 5 layers, classifiers of 49 and 101 columns -- through the drop-in CTC_Model against
oracle/ref_port.train_step in float64: log-probs, loss, every parameter gradient and the running statistics, with the reference-shaped
dropout masks of synth.train_case handed in.

Bounds: the exact mode's of tests/test_gpu_parity.py::test_train_step_split_bf16_variant -- log-probs 1e-4, loss 1e-5 relative,
gradients 2e-5 of scale outside the CNN, 3e-3 for conv.* weights, conv.bias only small -- for every mode run here: "f32x6" documents that
it meets mode 0's bounds, and "bf16x3" on a hidden size its persistent kernels are not built for IS mode 0's step (include/mdd_hip.h).
B * T >= 64 everywhere, so no shape needs that test's exemption for four-row batch statistics.  Distances are recorded under "geom_train_"."""
import functools

import numpy as np
import pytest
import torch

from tests import geometry_cases as gc
from tests.helpers import record_margin

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _cuda(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def _train_model(geom, sd):
    """test_gpu_parity._train_model's pattern; the drop-in class builds the reference's Embedding(44, 512), so a geometry with another
    table swaps the two text modules before the state_dict goes in (CTC_Model._config reads the table's shape from the module)."""
    import torch.nn as nn
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    model = CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=0.2)
    if (geom.emb_rows, geom.emb_dim) != (44, 512):
        model.embeds = nn.Embedding(geom.emb_rows, geom.emb_dim)
        model.lstm_embeds = nn.LSTM(geom.emb_dim, geom.hidden, batch_first=True, bidirectional=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return model.cuda().train()


@functools.lru_cache(maxsize=None)
def _case(name, B, T, L):
    """Inputs and the float64 step, once per geometry and shape for all modes."""
    from oracle import ref_port
    torch.set_num_threads(min(16, torch.get_num_threads()))
    geom = gc.geometry(gc.TRAIN[name][0])
    inputs = gc.train_case(geom, 300 + B, B, T, L)
    assert inputs[2].max() == geom.emb_rows - 1
    return geom, inputs, ref_port.train_step(*inputs, 0.2, dtype=torch.float64)


CASES = [(n, m, s) for n in sorted(gc.TRAIN) for m in gc.TRAIN[n][1] for s in gc.TRAIN_SHAPES]


@pytest.mark.parametrize("name,mode,shape", CASES, ids=["%s-%s-B%d" % (n, m, s[0]) for n, m, s in CASES])
def test_train_step_against_float64(name, mode, shape):
    from ctc_attention_mispronunciation_amd.train import CTCLoss
    B, T, L = shape
    assert B * T >= 64
    geom, (sd, x, x1, masks, tg, il, tl), (logp, loss, grads, run) = _case(name, B, T, L)
    model = _train_model(geom, sd)
    model.train_precision = mode
    model._dropout_masks = [torch.from_numpy(np.array(m, copy=True)) for m in masks]
    out = model(_cuda(x), _cuda(x1))
    assert out.shape == (T // 2, B, geom.num_class)
    e_logp = float(np.abs(out.detach().cpu().numpy().astype(np.float64) - logp).max())
    l2 = CTCLoss(reduction="sum")(out, torch.from_numpy(np.array(tg)), torch.from_numpy(np.array(il)), torch.from_numpy(np.array(tl))) / B
    e_loss = abs(float(l2.detach()) - loss) / abs(loss)
    l2.backward()
    params = dict(model.named_parameters())
    assert set(params) == set(grads), set(params) ^ set(grads)
    errs = sorted(((float(np.abs(p_.grad.cpu().numpy().astype(np.float64) - grads[k]).max()) / max(1.0, float(np.abs(grads[k]).max())), k)
                   for k, p_ in params.items() if not k.endswith("conv.bias")), reverse=True)
    outside = [(e, k) for e, k in errs if not k.startswith("conv.")]
    conv = [(e, k) for e, k in errs if k.startswith("conv.")]
    tag = "geom_train_%s_%s_B%d" % (name, mode, B)
    print(tag, "logp %.2e loss(rel) %.2e; grad err / scale, largest:" % (e_logp, e_loss), [(k, "%.1e" % e) for e, k in errs[:6]])
    record_margin(tag + "_logp", e_logp, TOL)
    record_margin(tag + "_loss_rel", e_loss, 1e-5)
    record_margin(tag + "_grad_worst", outside[0][0], 2e-5)
    record_margin(tag + "_grad_conv_worst", conv[0][0], 3e-3)
    assert e_logp <= TOL, (tag, e_logp)
    assert e_loss <= 1e-5, (tag, e_loss)
    for k, p_ in params.items():
        assert p_.grad is not None and bool(torch.isfinite(p_.grad).all()), k
        if k.endswith("conv.bias"):     # exactly zero in exact arithmetic (a bias in front of a batch-statistics BatchNorm): only smallness compares
            assert float(p_.grad.abs().max()) < 1e-3, (tag, k)
    for e, k in errs:
        assert e <= (3e-3 if k.startswith("conv.") else 2e-5), (tag, k, e)
    for k, b_ in model.named_buffers():
        if "running_" in k:
            np.testing.assert_allclose(b_.cpu().numpy(), run[k], rtol=0, atol=1e-5, err_msg=k)


ENGAGED = [n for n in sorted(gc.TRAIN) if "f32x6" in gc.TRAIN[n][1] and n != "feat120_H64_L2_C20"]


@pytest.mark.parametrize("name", ENGAGED)
def test_f32x6_runs_where_its_size_rule_passes(name):
    """The bounds above cannot tell mode 2 from mode 0 (it meets them by contract), so the dispatch is read from the bits.  At B = 4, T = 32
    layer 0's weight gradient dW_ih = DG^T . x is a contraction of M = 8H = 2048, N = 32 W2 >= 1952, K = 64 rows: it passes gemm_big's rule
    (2.6e8 multiply-adds >= 2^27, K >= 64) and must come out of the f32x6 kernels with other bits than the exact kernel's.  (The converse,
    equal bits where nothing passes the rule, is not asserted: the batch statistics are summed with fp64 atomics, whose order may move a
    float once in ~1e5 runs.)"""
    from ctc_attention_mispronunciation_amd.train import CTCLoss
    B, T, L = gc.TRAIN_SHAPES[0]
    geom, (sd, x, x1, masks, tg, il, tl), _ = _case(name, B, T, L)
    assert 8 * geom.hidden >= 128 and geom.rnn_in >= 128 and (T // 2) * B >= 64 and 8 * geom.hidden * geom.rnn_in * (T // 2) * B >= 1 << 27
    key, got = "rnns.0.rnn.weight_ih_l0", {}
    for mode in ("f32", "f32x6"):
        model = _train_model(geom, sd)
        model.train_precision = mode
        model._dropout_masks = [torch.from_numpy(np.array(m, copy=True)) for m in masks]
        out = model(_cuda(x), _cuda(x1))
        l2 = CTCLoss(reduction="sum")(out, torch.from_numpy(np.array(tg)), torch.from_numpy(np.array(il)), torch.from_numpy(np.array(tl))) / B
        l2.backward()
        got[mode] = dict(model.named_parameters())[key].grad.cpu()
    assert not torch.equal(got["f32"], got["f32x6"]), name
