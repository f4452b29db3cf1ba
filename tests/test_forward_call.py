"""The decode forward's entry points share one handle without seeing each other: mdd_forward, mdd_forward_fused and mdd_forward_raw each
carry their arguments in one value (csrc/model.h ForwardCall) instead of leaving them on the handle, a refused call leaves nothing
behind, the stage list mdd_forward_profile reports is the one mdd_forward runs, and the training handle reads its switches once."""
import ctypes as C

import numpy as np
import pytest
import torch

from ctc_attention_mispronunciation_amd import _lib, synth

pytestmark = pytest.mark.gpu

B, T_RAW, T, TP, L = 3, 30, 16, 8, 4
FRAMES, CANON = [8, 6, 3], [4, 2, 4]            # per-row T_g / 2 and L_g: rows shorter than T' and L
TINY = synth.TINY                               # mode 0, conv0 + conv1: forward_raw makes a stacked copy
FUSED = dict(feat=243, channels=32, hidden=256, layers=2, num_class=45)   # fused conv front end in modes 1 and 2: forward_raw is an index map


def _hip():
    from ctc_attention_mispronunciation_amd import hip_model
    return hip_model


def _inputs(geom, seed=5):
    """One device buffer whose address serves as x [B,T,F] of forward / forward_fused and as raw [B,T_raw,F/3] of forward_raw."""
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=T, L=L, seed=seed)
    buf = torch.from_numpy(np.ascontiguousarray(x)).cuda().reshape(-1)
    xv = buf.view(B, T, geom.feat)
    raw = buf[:B * T_RAW * (geom.feat // 3)].view(B, T_RAW, geom.feat // 3)
    assert xv.data_ptr() == raw.data_ptr() and _lib.lib().mdd_stack_len(T_RAW, 2, 2) == T
    frames = torch.tensor(FRAMES, dtype=torch.int32, device="cuda")
    canon = torch.tensor(CANON, dtype=torch.int32, device="cuda")
    return xv, raw, torch.from_numpy(x1).cuda(), frames, canon


def _call(m, what, inp, out):
    xv, raw, x1, frames, canon = inp
    if what == "forward":
        r = m.forward(xv, x1, out=out, sync_errors=True)
    elif what == "fused":
        r = m.forward_fused(xv, x1, frames, canon, out=out, sync_errors=True)
    else:
        r = m.forward_raw(raw, x1, out=out, sync_errors=True)
    assert r.data_ptr() == out.data_ptr()
    return r.cpu().numpy()


def _assert_same(what, got, want):
    if what == "fused":     # rows t >= frames[b] are undefined by the interface
        for b, n in enumerate(FRAMES):
            np.testing.assert_array_equal(got[:n, b], want[:n, b], err_msg="%s row %d" % (what, b))
    else:
        np.testing.assert_array_equal(got, want, err_msg=what)


@pytest.mark.parametrize("geom_kw,precision,graph", [(TINY, "f32", True), (TINY, "f32", False), (FUSED, "f32", True), (FUSED, "bf16x3", True),
                                                     (FUSED, "f32x6", True), (FUSED, "f32x6", False)],
                         ids=["tiny-f32", "tiny-f32-nograph", "fused-f32", "fused-bf16x3", "fused-f32x6", "fused-f32x6-nograph"])
def test_entry_points_on_one_handle_do_not_see_each_other(geom_kw, precision, graph, monkeypatch):
    """forward, fused, raw, forward, fused, raw on ONE handle, all on the same x address, x1, output buffer and B: every result equals, bit
    for bit, what a fresh handle returns that makes only that call (the arguments of one call must not colour the next: per-row lengths, the
    raw length, the captured graph found for the same addresses)."""
    if not graph:
        monkeypatch.setenv("MDD_GRAPH", "0")
    geom = synth.Geometry(**geom_kw)
    sd = synth.synth_state_dict(geom, seed=21)
    inp = _inputs(geom)
    out = torch.empty((TP, B, geom.num_class), dtype=torch.float32, device="cuda")
    want = {}
    for what in ("forward", "fused", "raw"):
        fresh = _hip().HipModel(geom, sd, precision=precision)
        assert fresh.precision == ("f32" if geom_kw is TINY else precision)
        want[what] = _call(fresh, what, inp, out)
        fresh.close()
    assert not np.array_equal(want["raw"], want["forward"])    # (the same bytes read as unstacked frames are another input)
    assert not np.array_equal(want["fused"][:FRAMES[1], 1], want["forward"][:FRAMES[1], 1])   # the per-row lengths do change row 1
    m = _hip().HipModel(geom, sd, precision=precision)
    for what in ("forward", "fused", "raw") * 2:
        out.fill_(float("nan"))
        _assert_same(what, _call(m, what, inp, out), want[what])


def test_a_refused_call_leaves_nothing_behind():
    """mdd_forward_fused without frames_dev and with an odd T, mdd_forward_raw with T_raw = 0: MDD_ERR_ARG, nothing enqueued (the output
    keeps its fill), and the next plain forward equals a fresh handle's bits."""
    lib = _lib.lib()
    geom = synth.Geometry(**FUSED)
    sd = synth.synth_state_dict(geom, seed=21)
    inp = _inputs(geom)
    xv, raw, x1, frames, canon = inp
    out = torch.empty((TP, B, geom.num_class), dtype=torch.float32, device="cuda")
    fresh = _hip().HipModel(geom, sd)
    want = _call(fresh, "forward", inp, out)
    fresh.close()
    m = _hip().HipModel(geom, sd)
    np.testing.assert_array_equal(_call(m, "forward", inp, out), want)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    st = _lib.current_stream_ptr()
    refused = [lambda: lib.mdd_forward_fused(m.handle, p(xv), B, T, p(x1), L, None, p(canon), p(out), st),
               lambda: lib.mdd_forward_fused(m.handle, p(xv), B, T - 1, p(x1), L, p(frames), p(canon), p(out), st),
               lambda: lib.mdd_forward_raw(m.handle, p(raw), B, 0, p(x1), L, p(out), st)]
    for k, call in enumerate(refused):
        out.fill_(-7.0)
        assert call() == -1, k                                  # MDD_ERR_ARG
        assert lib.mdd_sync(m.handle, st) == 0
        assert bool((out == -7.0).all()), k
        np.testing.assert_array_equal(_call(m, "forward", inp, out), want, err_msg=str(k))


@pytest.mark.parametrize("geom_kw,precision,lstm", [(TINY, "f32", None), (FUSED, "f32x6", None), (FUSED, "f32x6", "step"), (FUSED, "bf16x3", None)],
                         ids=["tiny", "fused-f32x6", "fused-f32x6-step", "fused-bf16x3"])
def test_stage_list(geom_kw, precision, lstm, monkeypatch):
    """mdd_forward_profile: 2 + 2 * layers + 6 stages, their names in model order, launch counts (the folded conv1 entry reports none; a
    recurrence reports one launch where the plan has a persistent layer kernel and one per step otherwise) and the closed-form flops of the
    geometry; a forward after the profile equals one before it."""
    if lstm:
        monkeypatch.setenv("MDD_LSTM", lstm)
    g = synth.Geometry(**geom_kw)
    sd = synth.synth_state_dict(g, seed=21)
    inp = _inputs(g)
    out = torch.empty((TP, B, g.num_class), dtype=torch.float32, device="cuda")
    m = _hip().HipModel(g, sd, precision=precision)
    before = _call(m, "forward", inp, out)
    prof = m.profile(inp[0], inp[2])
    torch.cuda.synchronize()
    fused = geom_kw is FUSED
    persistent = fused and lstm is None              # H = 256 has the persistent layer kernels; H = 8 and MDD_LSTM=step run step by step
    H, H2, ch, E, K0 = g.hidden, 2 * g.hidden, g.channels, g.emb_dim, g.rnn_in
    step = 2.0 * 2 * B * H * 4 * H
    want = [("conv_fused", 1, 2.0 * 9 * ch * B * TP * g.w2 * (ch + 6.0)), ("conv1_in_fused", 0, 0.0)] if fused else \
           [("conv0", 1, 2.0 * 9 * ch * B * T * g.w1), ("conv1", 1, 2.0 * 9 * ch * ch * B * TP * g.w2)]
    for n in range(g.layers):
        want.append(("gemm_ih%d" % n, 1, 2.0 * TP * B * 8 * H * (K0 if n == 0 else H2)))
        want.append(("lstm%d" % n, 1 if persistent else TP, step * TP))
    want += [("embed", 1, 0.0), ("gemm_text", 1, 2.0 * L * B * 8 * H * E), ("lstm_text", 1 if persistent else L, step * L),
             ("gemm_key", 1, 2.0 * L * B * H2 * H2), ("gemm_score", 1, 2.0 * B * TP * L * H2),
             ("attn_tail", 1, 2.0 * B * TP * (L * H2 + 2.0 * H2 * g.num_class))]
    assert len(want) == 2 + 2 * g.layers + 6 == _lib.lib().mdd_forward_num_stages(m.handle)
    assert [(name, launches, flops) for name, _, launches, flops in prof] == want
    for name, ms, launches, _ in prof:
        assert (ms > 0.0) == (launches > 0), name
    np.testing.assert_array_equal(_call(m, "forward", inp, out), before)


def test_training_switches_are_read_at_create(monkeypatch):
    """MDD_TRAIN_CONV1_IM2COL belongs to the training handle from its creation on: a handle created with it set and run after the variable
    is gone gives the gradients of one created and run with it set throughout (forward and backward of a step take the same conv1 path),
    within the gradient tolerance of tests/test_gpu_parity.py (_check_grads), at the smallest shape the training tests use."""
    from tests.test_gpu_parity import _train_model, _check_grads, _cuda
    from ctc_attention_mispronunciation_amd.train import CTCLoss, TrainHandle
    H, Bt, Tt, Lt = 256, 2, 4, 1
    geom = synth.Geometry(**dict(synth.REFERENCE, hidden=H))
    sd, x, x1, masks, tg, il, tl = synth.train_case(geom, 77, Bt, Tt, Lt, 1)

    def step(unset_after_create):
        monkeypatch.setenv("MDD_TRAIN_CONV1_IM2COL", "1")
        model = _train_model(geom, sd)
        model._train_handle = TrainHandle(model._config(), torch.cuda.current_device())
        if unset_after_create:
            monkeypatch.delenv("MDD_TRAIN_CONV1_IM2COL")
        model._dropout_masks = [torch.from_numpy(m) for m in masks]
        out = model(_cuda(x), _cuda(x1))
        loss = CTCLoss(reduction="sum")(out, torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)) / Bt
        loss.backward()
        return model, out.detach().cpu().numpy()
    ref, ref_logp = step(False)
    got, got_logp = step(True)
    np.testing.assert_allclose(got_logp, ref_logp, rtol=0, atol=1e-4)
    _check_grads(got, {k: p_.grad.cpu().numpy() for k, p_ in ref.named_parameters()})
