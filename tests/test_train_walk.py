"""ONE training handle, fixed weights, changing batch shapes (GPU): the walks of tests/train_walk_cases.py.  Every other training test builds
a fresh CTC_Model -- a fresh mdd_train_ws -- per shape and step; run_epoch drives one handle through hundreds of batches whose B, T and L
all change.  What one step leaves behind for the next (csrc/train.hip): grow-only buffers (a small step inside oversized ones), the split-K
partials and the K-padded bf16 operand planes shared by every contraction, hx / sync_words laid out differently by the persistent forward
and the persistent BPTT and carrying hand-off tags, the fp64 column sums shared by every BatchNorm site, and a kernel choice that flips
with the shape.

One test per (geometry, mode, order): at each shape the case's initial running statistics are copied back into the model's buffers in place
(the addresses the handle sees do not move), the case's masks handed in, forward, CTCLoss(sum) / B, backward --

* against the cached float64 step of oracle/ref_port.train_step at the bounds of tests/test_train_batch_tiles.py and test_train_geometry.py:
  log-probs 1e-4, loss 1e-5 relative, gradients 2e-5 of scale outside the CNN in "f32" and "f32x6" (and in "bf16x3" at H = 64, which must be
  mode 0's step); 5e-4, 1e-4, 2e-4 in "bf16x3" at H = 256; conv.* 3e-3, conv.bias < 1e-3, running statistics 1e-5 in every mode;
* against the same step on a FRESH model (fresh handle, same weights and masks, that shape only) at the exact mode's bounds for EVERY tensor,
  conv.* included (2e-5 of scale, no 3e-3 allowance: that one exists for ReLU gates flipping between fp32 and fp64, not between two runs of
  the same kernels; the only honest difference here is the order of the fp64 atomics).  This is what makes the walk sensitive in the CNN.
  The fresh step of a (geometry, mode, shape) is run once and shared by the orders.

After the last step h.sync() must raise nothing (a hand-off time-out of a persistent kernel surfaces there); the interleaved order ends on
its first shape again, which meets the same bounds as on its first visit.  The mixed-mode walk cycles train_precision f32 -> bf16x3 -> f32x6
per step on one handle, every step at its own mode's bounds (tests/test_train_f32x6.py covers only the switch 2 -> 0 at one shape).

Measured (profiles/train_walk_margins.json, "walk_train_*"): see DESIGN.md section 2."""
import numpy as np
import pytest
import torch

from tests import train_walk_cases as tw
from tests.helpers import record_margin

pytestmark = pytest.mark.gpu
EXACT, VARIANT = (1e-4, 1e-5, 2e-5), (5e-4, 1e-4, 2e-4)         # log-probs, loss (relative), gradients outside the CNN (of scale)
CONV_BOUND, RUN_BOUND = 3e-3, 1e-5


def bounds(name, mode):
    return VARIANT if mode == "bf16x3" and tw.geometry(name).hidden in (256, 384) else EXACT


def _cuda(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def make_model(geom, sd):
    import torch.nn as nn
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    model = CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=tw.P_DROP)
    if (geom.emb_rows, geom.emb_dim) != (44, 512):
        model.embeds = nn.Embedding(geom.emb_rows, geom.emb_dim)
        model.lstm_embeds = nn.LSTM(geom.emb_dim, geom.hidden, batch_first=True, bidirectional=True)
    model.load_state_dict({k: torch.from_numpy(np.array(v, copy=True)) for k, v in sd.items()})
    return model.cuda().train()


def gpu_step(model, mode, inp):
    """One forward / loss / backward of `model` on the case `inp`; returns (logp, loss, {key: grad}, {key: running statistic}) as float64 numpy."""
    from ctc_attention_mispronunciation_amd.train import CTCLoss
    sd, x, x1, masks, tg, il, tl = inp
    B, T = x.shape[0], x.shape[1]
    model.train_precision = mode
    model._dropout_masks = [torch.from_numpy(np.array(m, copy=True)) for m in masks]
    model.zero_grad(set_to_none=True)
    out = model(_cuda(x), _cuda(x1))
    assert out.shape == (T // 2, B, model.num_class)
    loss = CTCLoss(reduction="sum")(out, torch.from_numpy(np.array(tg)), torch.from_numpy(np.array(il)), torch.from_numpy(np.array(tl))) / B
    loss.backward()
    grads = {}
    for k, p_ in model.named_parameters():
        assert p_.grad is not None and bool(torch.isfinite(p_.grad).all()), k
        grads[k] = p_.grad.cpu().numpy().astype(np.float64)
    run = {k: b_.cpu().numpy().astype(np.float64) for k, b_ in model.named_buffers() if "running_" in k}
    return out.detach().cpu().numpy().astype(np.float64), float(loss.detach()), grads, run


def reset_running(model, sd):
    """The case's initial running statistics back into the model's own buffers: copy_, so no address the handle has seen moves."""
    with torch.no_grad():
        for k, b_ in model.named_buffers():
            if "running_" in k:
                b_.copy_(torch.from_numpy(np.array(sd[k], copy=True)))


def distances(got, ref):
    """(log-probs, loss relative, worst gradient outside the CNN, worst conv.* weight, worst conv.bias magnitude, running statistics,
    [(err of scale, key)] sorted) between two steps; `ref` gives the scales."""
    logp, loss, grads, run = got
    rlogp, rloss, rgrads, rrun = ref
    assert set(grads) == set(rgrads) and set(run) == set(rrun)
    errs = sorted(((float(np.abs(grads[k] - rgrads[k]).max()) / max(1.0, float(np.abs(rgrads[k]).max())), k) for k in grads), reverse=True)
    w = [(e, k) for e, k in errs if not k.endswith("conv.bias")]
    return dict(logp=float(np.abs(logp - rlogp).max()), loss=abs(loss - rloss) / abs(rloss),
                outside=max(e for e, k in w if not k.startswith("conv.")), conv=max(e for e, k in w if k.startswith("conv.")),
                conv_bias=max(float(np.abs(grads[k]).max()) for k in grads if k.endswith("conv.bias")),
                run=max(float(np.abs(run[k] - rrun[k]).max()) for k in run), errs=errs)


def check_against_float64(tag, d, bound):
    tol_logp, tol_loss, tol_grad = bound
    assert d["logp"] <= tol_logp, (tag, "logp", d["logp"])
    assert d["loss"] <= tol_loss, (tag, "loss", d["loss"])
    assert d["conv_bias"] < 1e-3, (tag, "conv.bias", d["conv_bias"])
    for e, k in d["errs"]:
        if not k.endswith("conv.bias"):
            assert e <= (CONV_BOUND if k.startswith("conv.") else tol_grad), (tag, k, e)
    assert d["run"] <= RUN_BOUND, (tag, "running statistics", d["run"])


def check_against_fresh(tag, d):
    assert d["logp"] <= EXACT[0], (tag, "logp", d["logp"])
    assert d["loss"] <= EXACT[1], (tag, "loss", d["loss"])
    for e, k in d["errs"]:                      # every tensor, conv.* weights and biases included
        assert e <= EXACT[2], (tag, k, e)
    assert d["run"] <= RUN_BOUND, (tag, "running statistics", d["run"])


_FRESH = {}


def fresh_step(name, mode, shape):
    """The step of a fresh model with its fresh handle on this shape alone; once per (geometry, mode, shape)."""
    key = (name, mode, shape)
    if key not in _FRESH:
        geom, inp, _ = tw.reference(name, shape)
        model = make_model(geom, inp[0])
        assert getattr(model, "_train_handle", None) is None
        _FRESH[key] = gpu_step(model, mode, inp)
        model._train_handle.sync()
        model._train_handle.close()
    return _FRESH[key]


def walk(name, order, modes, tag):
    """Drive one model (one handle) over `order`, step i in modes[i % len(modes)]; returns the worst distances of the walk."""
    geom = tw.geometry(name)
    model = make_model(geom, tw.state_dict(name))
    handle = None
    worst = {}
    for i, shape in enumerate(order):
        mode = modes[i % len(modes)]
        _, inp, ref = tw.reference(name, shape)
        reset_running(model, inp[0])
        got = gpu_step(model, mode, inp)
        if handle is None:
            handle = model._train_handle
        assert model._train_handle is handle and handle.handle, "the walk must stay on one handle"
        d64, dfr = distances(got, ref), distances(got, fresh_step(name, mode, shape))
        step = "%s step %d %s B%d T%d L%d" % (tag, i, mode, shape[0], shape[1], shape[2])
        print(step, "| float64: logp %.2e loss %.2e grad %.2e conv %.2e running %.2e | fresh: logp %.2e grad %.2e (%s) running %.2e"
              % (d64["logp"], d64["loss"], d64["outside"], d64["conv"], d64["run"], dfr["logp"], dfr["errs"][0][0], dfr["errs"][0][1], dfr["run"]))
        for k in ("logp", "loss", "outside", "conv", "run"):
            worst["f64_" + k] = max(worst.get("f64_" + k, 0.0), d64[k])
        worst["fresh_logp"] = max(worst.get("fresh_logp", 0.0), dfr["logp"])
        worst["fresh_grad"] = max(worst.get("fresh_grad", 0.0), dfr["errs"][0][0])
        worst["fresh_run"] = max(worst.get("fresh_run", 0.0), dfr["run"])
        check_against_float64(step, d64, bounds(name, mode))
        check_against_fresh(step, dfr)
    handle.sync()                   # raises what a persistent kernel flagged (a hand-off time-out) or an index error
    return worst


def _record(tag, worst, bound):
    record_margin(tag + "_logp", worst["f64_logp"], bound[0])
    record_margin(tag + "_loss_rel", worst["f64_loss"], bound[1])
    record_margin(tag + "_grad_worst", worst["f64_outside"], bound[2])
    record_margin(tag + "_grad_conv_worst", worst["f64_conv"], CONV_BOUND)
    record_margin(tag + "_running_stats", worst["f64_run"], RUN_BOUND)
    record_margin(tag + "_vs_fresh_logp", worst["fresh_logp"], EXACT[0])
    record_margin(tag + "_vs_fresh_grad_worst", worst["fresh_grad"], EXACT[2])
    record_margin(tag + "_vs_fresh_running_stats", worst["fresh_run"], RUN_BOUND)


CASES = [(n, m, o) for n in tw.GEOMS for m in tw.MODES[n] for o in ("up", "down", "mixed")]


@pytest.mark.parametrize("name,mode,order", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_walk_one_handle_against_float64_and_fresh(name, mode, order):
    tag = "walk_train_%s_%s_%s" % (name, mode, order)
    worst = walk(name, tw.walk_orders(name)[order], (mode,), tag)
    _record(tag, worst, bounds(name, mode))


def test_walk_mixed_modes_on_one_handle():
    """The interleaved order of H256_L1 with the mode cycling f32 -> bf16x3 -> f32x6 per step: each step at its own mode's bounds.  The
    distances recorded are the walk's worst, against the variant's (widest) bounds."""
    name, tag = "H256_L1", "walk_train_H256_L1_cycled_mixed"
    worst = walk(name, tw.walk_orders(name)["mixed"], ("f32", "bf16x3", "f32x6"), tag)
    _record(tag, worst, VARIANT)
