"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the committed goldens.
Tolerances: log-probs within 1e-4 absolute (BASELINE.json north_star); decoded ids / alignments exact."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from tests.helpers import npz, jload, ids_to_beam_string, ids_to_greedy_string, GOLD
from ctc_attention_mispronunciation_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _hip():
    from ctc_attention_mispronunciation_amd import hip_model
    return hip_model


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_forward_tiny_every_stage():
    g = npz("g1_tiny.npz")
    geom = synth.Geometry(**synth.TINY)
    sd = synth.synth_state_dict(geom, seed=11)
    m = _hip().HipModel(geom, sd, taps=True)
    logp = m.forward(_cuda(g["x"]), _cuda(g["x1"]), sync_errors=True).cpu().numpy()
    B, T = g["x"].shape[:2]
    L = g["x1"].shape[1]
    conv1 = m.tap("conv1").cpu().numpy().reshape(T // 2, B, geom.channels, -1).transpose(1, 2, 0, 3)
    np.testing.assert_allclose(conv1, g["conv1"], rtol=0, atol=TOL)
    for i in range(geom.layers):
        np.testing.assert_allclose(m.tap("rnn%d" % i).cpu().numpy().reshape(T // 2, B, -1), g["rnn%d" % i], rtol=0, atol=TOL)
    np.testing.assert_allclose(m.tap("text").cpu().numpy().reshape(L, B, -1).transpose(1, 0, 2), g["text"], rtol=0, atol=TOL)
    np.testing.assert_allclose(m.tap("key").cpu().numpy().reshape(L, B, -1).transpose(1, 0, 2), g["key"], rtol=0, atol=TOL)
    np.testing.assert_allclose(logp, g["logp"], rtol=0, atol=TOL)
    np.testing.assert_allclose(logp, oracle.forward(sd, g["x"], g["x1"]), rtol=0, atol=TOL)


@pytest.mark.parametrize("precision", ["f32", "f32x6", "bf16x3"])
@pytest.mark.parametrize("idx", [0, 1, 2])
def test_forward_reference_geometry_golden(idx, precision):
    meta = jload("g2_ref.json")[idx]
    ref = npz("g2_ref.npz")[meta["tag"] + "_logp"]
    geom = synth.Geometry(**meta["geom"])
    sd = synth.synth_state_dict(geom, seed=meta["seed"])
    x, x1, _, _ = synth.synth_batch(geom, B=meta["B"], T=meta["T"], L=meta["L"], seed=meta["seed"])
    m = _hip().HipModel(geom, sd, precision=precision, taps=True)
    assert m.precision == precision
    logp = m.forward(_cuda(x), _cuda(x1)).cpu().numpy()
    np.testing.assert_allclose(logp, ref, rtol=0, atol=TOL)
    print("%s %s: max|logp - reference| = %.2e" % (meta["tag"], precision, np.abs(logp - ref).max()))
    from tests.helpers import record_margin
    record_margin("g2_%s_%s_logp" % (meta["tag"], precision), float(np.abs(logp - ref).max()), TOL)
    # stage taps against the oracle (conv1 / key exist only as split-bf16 planes in bf16x3 mode)
    taps = {}
    oracle.forward(sd, x, x1, taps)
    B, T, L = meta["B"], meta["T"], meta["L"]
    conv1 = m.tap("conv1").cpu().numpy().reshape(T // 2, B, geom.channels, -1).transpose(1, 2, 0, 3)
    np.testing.assert_allclose(conv1, taps["conv1"], rtol=0, atol=TOL)
    for i in range(geom.layers):
        np.testing.assert_allclose(m.tap("rnn%d" % i).cpu().numpy().reshape(T // 2, B, -1), taps["rnn%d" % i], rtol=0, atol=TOL)
    np.testing.assert_allclose(m.tap("key").cpu().numpy().reshape(L, B, -1).transpose(1, 0, 2), taps["key"], rtol=0, atol=TOL)
    if meta["min_top2_gap"] > 1e-3:
        assert (logp.argmax(-1) == ref.argmax(-1)).all()
    # graph replay gives the same bits
    again = m.forward(_cuda(x), _cuda(x1)).cpu().numpy()
    np.testing.assert_array_equal(logp, again)


def test_dropin_class_matches_golden_and_reference_api():
    """The reference-shaped class: same constructor, state_dict keys, forward signature."""
    import torch.nn as nn
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    meta = jload("g2_ref.json")[0]
    ref = npz("g2_ref.npz")[meta["tag"] + "_logp"]
    geom = synth.Geometry(**meta["geom"])
    sd = synth.synth_state_dict(geom, seed=meta["seed"])
    model = CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=0.2)
    assert set(model.state_dict().keys()) == set(sd.keys())
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.eval()
    x, x1, _, _ = synth.synth_batch(geom, B=meta["B"], T=meta["T"], L=meta["L"], seed=meta["seed"])
    with torch.no_grad():
        out_cpu_in = model(torch.from_numpy(x), torch.from_numpy(x1))          # CPU tensors in -> CPU tensor out
        out_gpu_in = model(torch.from_numpy(x).cuda(), torch.from_numpy(x1).cuda())
    assert not out_cpu_in.is_cuda and out_gpu_in.is_cuda
    np.testing.assert_allclose(out_cpu_in.numpy(), ref, rtol=0, atol=TOL)
    np.testing.assert_array_equal(out_cpu_in.numpy(), out_gpu_in.cpu().numpy())
    bad = torch.from_numpy(x1).clone()
    bad[0, 0] = 44                                                               # 'err' cannot be embedded (model_ctc.py:149)
    with pytest.raises(IndexError):
        model(torch.from_numpy(x), bad)


@pytest.mark.parametrize("precision", ["f32", "f32x6", "bf16x3"])
def test_forward_full_size_properties(precision):
    """BASELINE config size (B=64, 10 s): rows are distributions; an utterance's posteriors do not depend on
    the other utterances of the batch (eval mode has no cross-batch op), bit for bit; and a 2-utterance
    slice agrees with the CPU oracle."""
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=1234)
    x, x1, _, _ = synth.synth_batch(geom, B=64, T=500, L=40, seed=1234, ragged=True)
    m = _hip().HipModel(geom, sd, precision=precision)
    logp = m.forward(_cuda(x), _cuda(x1))
    assert logp.shape == (250, 64, 45)
    s = torch.exp(logp.double()).sum(-1)
    assert float((s - 1).abs().max()) < 1e-5
    sub = [3, 40]
    lp2 = m.forward(_cuda(x[sub]), _cuda(x1[sub]))
    np.testing.assert_array_equal(lp2.cpu().numpy(), logp[:, sub, :].cpu().numpy())
    ref = oracle.forward(sd, x[sub][:, :120], x1[sub])      # bounded slice for the scalar oracle (T=120)
    lp3 = m.forward(_cuda(np.ascontiguousarray(x[sub][:, :120])), _cuda(x1[sub])).cpu().numpy()
    np.testing.assert_allclose(lp3, ref, rtol=0, atol=TOL)
    print("full-size slice %s: max|logp - oracle| = %.2e" % (precision, np.abs(lp3 - ref).max()))


@pytest.mark.parametrize("si", [0, 1])
def test_decoders_golden(si, tmp_path):
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import GreedyDecoder, BeamDecoder
    meta = jload("g3_decode.json")["sets"][si]
    g = npz("g3_decode.npz")
    Cn = meta["C"]
    i2c = dict(enumerate(meta["int2char"]))
    greedy = GreedyDecoder(i2c, space_idx=-1, blank_index=0)
    beams = {}
    for r in meta["records"]:
        lp = torch.from_numpy(g["c%d_case%d" % (Cn, r["case"])]).unsqueeze(1)
        assert greedy.decode(lp, [r["len"]])[0] == r["greedy"], r
        key = (r["alpha"], r["width"])
        if key not in beams:
            beams[key] = BeamDecoder(i2c, beam_width=r["width"], blank_index=0, space_idx=-1,
                                     lm_path=os.path.join(GOLD, "lm_synth%d.arpa" % Cn), lm_alpha=r["alpha"])
            np.testing.assert_array_equal(beams[key].lm.dense_table(i2c, Cn), g["lm%d" % Cn])
        assert r["error"] is None
        assert beams[key].decode(lp.cuda(), [r["len"]])[0] == r["beam"], r
    for f in meta["failures"]:
        lp = torch.from_numpy(g["c%d_fail_%s" % (Cn, f["name"])]).unsqueeze(1)
        bd = BeamDecoder(i2c, beam_width=f["width"], blank_index=0, space_idx=-1,
                         lm_path=os.path.join(GOLD, f["lm"].replace("lm", "lm_synth") + ".arpa"), lm_alpha=f["alpha"])
        with pytest.raises({"IndexError": IndexError, "ValueError": ValueError, "KeyError": KeyError}[f["error"]]):
            bd.decode(lp, [f["len"]])
        assert greedy.decode(lp, [f["len"]])[0] == f["greedy"]
    b = meta["batch"]
    batch = torch.from_numpy(g["c%d_batch" % Cn])
    assert greedy.decode(batch, b["lens"]) == b["greedy"]
    assert beams[(0.0, 10)].decode(batch.cuda(), b["lens"]) == b["beam"]


def test_decoders_full_size_against_oracle():
    """B=64 x 250 frames: model-like flat posteriors and the 'peaky' set of SURVEY.md §8(d); ids must equal
    the oracle's exactly, scores to 1e-7 relative."""
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import GreedyDecoder, BeamDecoder
    Cn, T, B = 45, 250, 64
    i2c = synth.phone_table_41()
    rs = np.random.Generator(np.random.PCG64(7))
    lens = [T] + [int(v) for v in rs.integers(T // 2, T + 1, size=B - 1)]
    bd = BeamDecoder(i2c, beam_width=10, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=0.0)
    table = bd.lm.dense_table(i2c, Cn)
    for kind in ("peaky", "flat"):
        if kind == "peaky":
            lp = np.stack([synth.peaky_logp(T, Cn, 35, seed=100 + b) for b in range(B)], axis=1)
        else:
            z = rs.standard_normal((T, B, Cn)).astype(np.float32)
            lp = torch.log_softmax(torch.from_numpy(z), -1).numpy()
        ids, nids = GreedyDecoder(i2c, space_idx=-1, blank_index=0).decode_ids(torch.from_numpy(lp).cuda(), lens)
        ids, nids = ids.cpu().numpy(), nids.cpu().numpy()
        assert [ids[b, :nids[b]].tolist() for b in range(B)] == oracle.greedy(lp, lens)
        ids, nids, st, sc = bd.decode_ids(torch.from_numpy(lp).cuda(), lens)
        want, wst, wsc = oracle.beam(lp, lens, table, return_scores=True)
        assert not st.cpu().numpy().any() and not wst.any()
        ids, nids = ids.cpu().numpy(), nids.cpu().numpy()
        assert [ids[b, :nids[b]].tolist() for b in range(B)] == want, kind
        # scores: the two sides round exp(logp) to fp32 with different libm's (<= 1 ulp apart on ~1% of entries)
        np.testing.assert_allclose(sc.cpu().numpy(), wsc, rtol=1e-7)


def test_ctc_loss_golden_and_oracle():
    g = npz("g5_ctc.npz")
    for meta in jload("g5_ctc.json"):
        i = meta["i"]
        nll, grad = _hip().ctc_loss(_cuda(g["logp%d" % i]), _cuda(g["tg%d" % i]), _cuda(g["il%d" % i]), _cuda(g["tl%d" % i]))
        nll, grad = nll.cpu().numpy(), grad.cpu().numpy()
        ref_nll, ref_grad = g["nll%d" % i], g["grad%d" % i]
        fin = np.isfinite(ref_nll)
        assert (np.isinf(nll) == ~fin).all()
        np.testing.assert_allclose(nll[fin], ref_nll[fin], rtol=2e-6, atol=1e-4)
        np.testing.assert_allclose(grad[:, fin, :], ref_grad[:, fin, :], rtol=0, atol=TOL)
        onll, ograd = oracle.ctc_loss(g["logp%d" % i], g["tg%d" % i], g["il%d" % i], g["tl%d" % i])
        np.testing.assert_allclose(grad[:, fin, :], ograd[:, fin, :], rtol=0, atol=2e-6)
    # BASELINE config (5) shard size: B=32, T'=250, L=40
    rs = np.random.Generator(np.random.PCG64(12))
    T, B, Cn, L = 250, 32, 45, 40
    lp = torch.log_softmax(torch.from_numpy(rs.standard_normal((T, B, Cn)).astype(np.float32)), -1).numpy()
    tg = rs.integers(1, Cn, size=(B, L))
    il = rs.integers(2 * L + 1, T + 1, size=B); il[0] = T
    tl = rs.integers(L // 2, L + 1, size=B); tl[0] = L
    nll, grad = _hip().ctc_loss(_cuda(lp), _cuda(tg), _cuda(il), _cuda(tl))
    onll, ograd = oracle.ctc_loss(lp, tg, il, tl)
    np.testing.assert_allclose(nll.cpu().numpy(), onll, rtol=1e-6)
    np.testing.assert_allclose(grad.cpu().numpy(), ograd, rtol=0, atol=2e-6)
    # linearity property: sum over classes of the deposited gradient is 0 on every live frame
    assert float(grad.sum(-1).abs().max()) < 1e-4


def test_stack_skip_golden():
    from ctc_attention_mispronunciation_amd.utils.data_loader import stack_features
    g = npz("g6_input.npz")
    for i in range(6):
        np.testing.assert_array_equal(stack_features(torch.from_numpy(g["raw%d" % i])).cpu().numpy(), g["stk%d" % i])
    raw = synth.synth_raw_features(4, T_raw=1000)
    out = stack_features(torch.from_numpy(raw)).cpu().numpy()
    assert out.shape == (4, 500, 243)
    for b in range(4):
        np.testing.assert_array_equal(out[b], oracle.stack_skip(raw[b]))


def test_persistent_lstm_equals_step_kernels_bitwise(monkeypatch):
    """The persistent team-synchronised layer kernel and the per-step split-bf16 kernel issue the same MFMAs in the
    same order, so their outputs must be identical bit for bit -- at a fused batch size, full length, with the
    consumer CUs' caches warm (the hand-off is re-run 3 times)."""
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=1234)
    x, x1, _, _ = synth.synth_batch(geom, B=160, T=500, L=40, seed=99, ragged=True)
    monkeypatch.setenv("MDD_LSTM", "x3")
    ref = _hip().HipModel(geom, sd, precision="bf16x3").forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    monkeypatch.delenv("MDD_LSTM")
    m = _hip().HipModel(geom, sd, precision="bf16x3")
    for _ in range(3):
        got = m.forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
        np.testing.assert_array_equal(got, ref)


# ---------------------------------------------------------------------------- edge cases
@pytest.mark.parametrize("B,T,L", [(1, 2, 1), (1, 8, 3), (17, 8, 5), (33, 6, 2)])
@pytest.mark.parametrize("precision", ["f32", "f32x6", "bf16x3"])
def test_forward_edge_shapes_against_oracle(B, T, L, precision):
    """Smallest legal input (one output frame, one canonical phoneme), batch sizes that are not multiples of the
    MFMA tile, ragged padding -- reference geometry, against the CPU oracle."""
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=4321)
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=T, L=L, seed=B * 100 + T, ragged=True)
    m = _hip().HipModel(geom, sd, precision=precision)
    got = m.forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    np.testing.assert_allclose(got, oracle.forward(sd, x, x1), rtol=0, atol=TOL)


@pytest.mark.parametrize("H", [384, 256])
@pytest.mark.parametrize("B", [17, 100, 256, 300, 512, 513, 700, 1000, 1024])
def test_persistent_lstm_batch_sizes_match_step_kernels(B, H, monkeypatch):
    """Every team geometry of the persistent BiLSTM (1 to 4 row tiles per team), H = 384 and H = 256, against the per-step
    split-bf16 kernels, bit for bit; short sequence, full width."""
    geom = synth.Geometry(**dict(synth.REFERENCE, hidden=H))
    sd = synth.synth_state_dict(geom, seed=77)
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=40, L=6, seed=B, ragged=True)
    monkeypatch.setenv("MDD_LSTM", "x3")
    ref = _hip().HipModel(geom, sd, precision="bf16x3").forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    monkeypatch.delenv("MDD_LSTM")
    got = _hip().HipModel(geom, sd, precision="bf16x3").forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("H", [384, 256])
@pytest.mark.parametrize("B", [17, 100, 256, 300, 512, 513, 700, 1000, 1024])
def test_persistent_f32_lstm_batch_sizes_match_step_kernels(B, H, monkeypatch):
    """The reference-width persistent BiLSTM (lstm_layer_f32_kernel: exact fp32 MFMA, W_hh resident in registers) in every team
    geometry (1 to 4 row tiles per team), H = 384 and H = 256, against one lstm_step_packed_kernel launch per step: bit for bit,
    taps of every layer included; ragged lengths exercise the reverse direction's per-row start."""
    geom = synth.Geometry(**dict(synth.REFERENCE, hidden=H))
    sd = synth.synth_state_dict(geom, seed=77)
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=40, L=6, seed=B, ragged=True)
    monkeypatch.setenv("MDD_LSTM", "step")
    m0 = _hip().HipModel(geom, sd, precision="f32", taps=True)
    ref = m0.forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    ref_taps = [m0.tap("rnn%d" % i).cpu().numpy() for i in range(4)] + [m0.tap("text").cpu().numpy()]
    monkeypatch.delenv("MDD_LSTM")
    m1 = _hip().HipModel(geom, sd, precision="f32", taps=True)
    got = m1.forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    for i, name in enumerate(["rnn0", "rnn1", "rnn2", "rnn3", "text"]):
        np.testing.assert_array_equal(m1.tap(name).cpu().numpy(), ref_taps[i], err_msg=name)
    np.testing.assert_array_equal(got, ref)


def test_persistent_f32_lstm_full_length_and_poisoned_input(monkeypatch):
    """T' = 250 at the benchmarked batch (two row tiles per team) against the step kernels, bit for bit; then one utterance gets a NaN
    and an Inf frame: the launch neither stalls nor reports an error (the tagged hand-off keeps valid tags whatever the state holds),
    and every other utterance's rows are untouched."""
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=79)
    x, x1, _, _ = synth.synth_batch(geom, B=512, T=500, L=40, seed=3, ragged=False)
    monkeypatch.setenv("MDD_LSTM", "step")
    ref = _hip().HipModel(geom, sd, precision="f32").forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    monkeypatch.delenv("MDD_LSTM")
    m = _hip().HipModel(geom, sd, precision="f32")
    got = m.forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    np.testing.assert_array_equal(got, ref)
    xb = x.copy()
    xb[37, 100, 5] = np.nan
    xb[37, 300, 7] = np.inf
    bad = m.forward(_cuda(xb), _cuda(x1), sync_errors=True).cpu().numpy()
    keep = [b for b in range(512) if b != 37]
    np.testing.assert_array_equal(bad[:, keep], ref[:, keep])


@pytest.mark.parametrize("H", [384, 256])
@pytest.mark.parametrize("B", [1, 17, 100, 128, 129, 256, 300, 512, 513, 700, 1000, 1024])
def test_persistent_x6_lstm_tracks_exact_fp32_recurrence(B, H, monkeypatch):
    """The default mode's recurrence (lstm_layer_x6_kernel: W_hh' and h as three bf16 planes each, six products, teams of 16) in every
    team geometry (1 to 8 row tiles per team), H = 384 and H = 256, beside the same mode run with the exact-fp32 layer kernel
    (MDD_LSTM_X6=0; everything else identical): every layer's raw state within 1e-6 absolute (|h| <= 1; the products differ by
    ~2^-24 relative per term and in summation order; measured 2.4e-7), the log-probs within 1e-5; ragged lengths exercise the reverse direction's
    per-row start, and the padded frames of short rows are exact zeros in both.  Two runs of the x6 kernel are bit-identical."""
    geom = synth.Geometry(**dict(synth.REFERENCE, hidden=H))
    sd = synth.synth_state_dict(geom, seed=77)
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=40, L=6, seed=B, ragged=True)
    monkeypatch.setenv("MDD_LSTM_X6", "0")
    m0 = _hip().HipModel(geom, sd, precision="f32x6", taps=True)
    ref = m0.forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    ref_taps = [m0.tap("rnn%d" % i).cpu().numpy() for i in range(4)] + [m0.tap("text").cpu().numpy()]
    monkeypatch.setenv("MDD_LSTM_X6", "force")                  # (the library's own choice leaves H = 256 beyond 128 rows to the exact-fp32 kernel: it is the faster one there)
    m1 = _hip().HipModel(geom, sd, precision="f32x6", taps=True)
    got = m1.forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    worst = 0.0
    for i, name in enumerate(["rnn0", "rnn1", "rnn2", "rnn3", "text"]):
        t = m1.tap(name).cpu().numpy()
        assert np.isfinite(t).all(), name
        np.testing.assert_array_equal(t == 0, ref_taps[i] == 0, err_msg=name + ": zero pattern (padded frames)")
        worst = max(worst, float(np.abs(t - ref_taps[i]).max()))
        np.testing.assert_allclose(t, ref_taps[i], rtol=0, atol=1e-6, err_msg=name)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-5)
    from tests.helpers import record_margin
    record_margin("x6_recurrence_vs_exact_fp32_state[B=%d,H=%d]" % (B, H), worst, 1e-6)
    again = m1.forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    np.testing.assert_array_equal(again, got)


@pytest.mark.parametrize("B", [256, 512, 640])
def test_persistent_x6_lstm_redo_branch(B, monkeypatch):
    """A panel whose granules have not all arrived is fetched again and the tile's products are recomputed -- a branch that real runs take
    in < 0.1 % of the phases.  MDD_X6_FORCE_REDO=4 declares every fourth phase stale (two, four and five tiles per team: the plain and
    the skewed schedule): the posteriors must not change by a bit."""
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=81)
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=120, L=9, seed=B, ragged=True)
    ref = _hip().HipModel(geom, sd, precision="f32x6").forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    monkeypatch.setenv("MDD_X6_FORCE_REDO", "4")
    got = _hip().HipModel(geom, sd, precision="f32x6").forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    np.testing.assert_array_equal(got, ref)


def test_persistent_x6_lstm_full_length_and_poisoned_input(monkeypatch):
    """T' = 250 at the benchmarked batch (four row tiles per team) beside the exact-fp32 layer kernel; then one utterance gets a NaN
    and an Inf frame: the launch neither stalls nor reports an error (a NaN state travels as 1.5, which keeps the tag bits valid),
    and every other utterance's rows are bit-identical to the clean run."""
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=79)
    x, x1, _, _ = synth.synth_batch(geom, B=512, T=500, L=40, seed=3, ragged=False)
    monkeypatch.setenv("MDD_LSTM_X6", "0")
    ref = _hip().HipModel(geom, sd, precision="f32x6").forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    monkeypatch.delenv("MDD_LSTM_X6")
    m = _hip().HipModel(geom, sd, precision="f32x6")
    got = m.forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=0, atol=5e-5)
    from tests.helpers import record_margin
    record_margin("x6_recurrence_vs_exact_fp32_logprobs[B=512,T'=250]", float(np.abs(got - ref).max()), 5e-5)
    xb = x.copy()
    xb[37, 100, 5] = np.nan
    xb[37, 300, 7] = np.inf
    bad = m.forward(_cuda(xb), _cuda(x1), sync_errors=True).cpu().numpy()
    keep = [b for b in range(512) if b != 37]
    np.testing.assert_array_equal(bad[:, keep], got[:, keep])


def _gemm_modes_against_fp64(M, N, K, modes, seed=0):
    import ctypes as C
    from ctc_attention_mispronunciation_amd import _lib
    L = _lib.lib()
    L.mdd_diag_gemm.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K)).astype(np.float32)
    A[A < 0] = 0.0                                               # post-ReLU / BatchNorm-like operands
    A[:, ::7] *= 30.0
    W = (rng.uniform(-1, 1, (N, K)) * 0.05).astype(np.float32)
    ref = A.astype(np.float64) @ W.astype(np.float64).T
    out = {"aten_f32": (torch.from_numpy(A) @ torch.from_numpy(W).T).numpy()}
    Ad, Wd = _cuda(A), _cuda(W)
    for name, mode in modes:
        Cd = torch.empty((M, N), device="cuda")
        assert L.mdd_diag_gemm(mode, Ad.data_ptr(), Wd.data_ptr(), Cd.data_ptr(), M, N, K, None) == 0, L.mdd_last_error().decode()
        torch.cuda.synchronize()
        out[name] = Cd.cpu().numpy()
    scale = float(np.sqrt((ref ** 2).mean()))
    return {k: (float(np.abs(v - ref).max()) / scale, float(np.abs(v - ref).mean()) / scale) for k, v in out.items()}


@pytest.mark.parametrize("M,N,K", [(1024, 768, 1952), (1500, 3072, 768), (2048, 512, 512)])
def test_gemm_f32x6_accuracy(M, N, K):
    """One GEMM of the model's shapes through every arithmetic of the library against the float64 product, beside ATen's fp32 GEMM on
    the CPU: the f32x6 form (three bf16 planes per operand = all 24 significand bits, six products, hi.hi in an accumulator of its
    own) must be at least as close to float64 as ATen's fp32 -- the condition under which it stands in for fp32 arithmetic -- and
    closer than the exact-fp32 MFMA kernel (one accumulation chain over K); split-bf16 x3 (16 significand bits) is two orders worse."""
    from tests.helpers import record_margin
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    r = _gemm_modes_against_fp64(M, N, K, [("mfma_f32", 0), ("bf16x3", 1), ("f32x6", 3)], seed=K)
    print("GEMM %dx%dx%d, |C - C64| / rms(C64), max and mean: " % (M, N, K) + "; ".join("%s %.2e %.2e" % (k, v[0], v[1]) for k, v in r.items()))
    for k, v in r.items():
        record_margin("gemm_%dx%dx%d_%s_mean_rel" % (M, N, K, k), v[1])
    assert r["f32x6"][1] <= r["aten_f32"][1] and r["f32x6"][0] <= 1.5 * r["aten_f32"][0]
    assert r["f32x6"][1] < r["mfma_f32"][1] < r["bf16x3"][1]


def test_gate_functions_accuracy():
    """The short sigmoid / tanh of the reference-width recurrences (hardware exp2 / rcp + one Newton step; odd polynomial below
    |v| = 1/4) against float64 on a dense sweep and on the special values: they stay at fp32 working accuracy -- the bound asserted
    is 2 ulp of the result for sigmoid on [0, 8], 1e-7 absolute everywhere, and 4 ulp for tanh (measured values printed), where ATen's
    Sleef kernels give ~1 ulp -- and hold their limits at the ends of the range."""
    import ctypes as C
    from ctc_attention_mispronunciation_amd import _lib
    L = _lib.lib()
    L.mdd_diag_gates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-20, 20, 400000), rng.uniform(-1, 1, 400000), rng.uniform(-0.3, 0.3, 200000),
                        rng.standard_normal(200000) * 1e-3, np.linspace(0.2499, 0.2501, 2001),
                        [0.0, -0.0, 0.25, -0.25, 1e-30, -1e-30, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4, 3e38, -3e38, np.inf, -np.inf]]).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    sg, th = torch.empty_like(xd), torch.empty_like(xd)
    assert L.mdd_diag_gates(xd.data_ptr(), sg.data_ptr(), th.data_ptr(), x.size, None) == 0, L.mdd_last_error().decode()
    torch.cuda.synchronize()
    sg, th = sg.cpu().numpy(), th.cpu().numpy()
    x64 = x.astype(np.float64)
    with np.errstate(over="ignore"):
        sref, tref = 1.0 / (1.0 + np.exp(-x64)), np.tanh(x64)
    assert np.isfinite(sg).all() and np.isfinite(th).all()
    big = np.abs(x64) >= 1e-20
    ulp_s = np.abs(sg - sref) / np.spacing(np.maximum(sref, 1e-30).astype(np.float32))
    ulp_t = np.abs(th - tref)[big] / np.spacing(np.abs(tref[big]).astype(np.float32))
    pos, neg = (x64 >= 0) & (x64 <= 8.0), (x64 < 0) & (x64 >= -8.0)
    # sigmoid's argument product v * log2(e) is rounded once, so for v < 0 the RELATIVE error of the (small) result grows with |v|
    # (~0.7 |v| ulp); what the cell update consumes is the absolute value, bounded below over the whole range
    print("gate functions: sigmoid max %.2f ulp (mean %.3f) on [0, 8], %.2f ulp (mean %.3f) on [-8, 0), max |err| %.2e overall; tanh max %.2f ulp (mean %.3f), max |err| %.2e"
          % (ulp_s[pos].max(), ulp_s[pos].mean(), ulp_s[neg].max(), ulp_s[neg].mean(), np.abs(sg - sref).max(), ulp_t.max(), ulp_t.mean(), np.abs(th - tref).max()))
    assert ulp_s[pos].max() <= 2.0 and ulp_s[neg].max() <= 10.0 and ulp_t.max() <= 4.0
    assert (np.abs(sg - sref) <= 1e-7).all() and (np.abs(th - tref) <= 2e-7).all()
    assert (th[~big] == x[~big]).all()                            # tanh(v) = v to the last bit for tiny v, signed zeros kept
    # (sigmoid's exponent is capped at 2^126 so that the Newton step never sees an infinity: its lower limit is 2^-126, not 0)
    assert sg[x == np.inf][0] == 1.0 and sg[x == -np.inf][0] <= 1.2e-38 and th[x == np.inf][0] == 1.0 and th[x == -np.inf][0] == -1.0
    nan = torch.full((4,), float("nan")).cuda()
    s2, t2 = torch.empty_like(nan), torch.empty_like(nan)
    assert L.mdd_diag_gates(nan.data_ptr(), s2.data_ptr(), t2.data_ptr(), 4, None) == 0
    assert torch.isnan(s2).all() and torch.isnan(t2).all()


def test_sched_hints_do_not_change_results():
    """Round 2's finding: with the __builtin_amdgcn_sched_barrier calls removed from lstm_layer_granule_kernel its results moved (1.7e-4 on an
    rnn tap).  Cause (profiles/round3_lstm_ordering.txt): a builtin MFMA followed back to back by an inline-asm MFMA on the same accumulator --
    the compiler cannot see the asm one's read and inserts no wait state; the barriers happened to keep the product-major order that spaces
    them.  All product-loop MFMAs are asm volatile now (issue order = source order), so the barriers are a speed hint only: the library's
    twin built WITHOUT them (libmdd_hip_nohint.so, `make nohint`) must give the bits of the library itself -- reference geometry golden
    shape, one to four row tiles per team (B = 100, 512, 700, 1000), H = 384 and 256, the training variant's forward included."""
    import subprocess
    import sys
    from tests.helpers import ROOT
    twin = os.path.join(ROOT, "ctc-attention-mispronunciation_amd", "libmdd_hip_nohint.so")
    assert os.path.exists(twin), "build it with `make -C ctc-attention-mispronunciation_amd/csrc nohint` (__graft_entry__.build() does)"
    code = r"""
import sys, hashlib, numpy as np, torch
sys.path.insert(0, %r)
from ctc_attention_mispronunciation_amd import synth
from ctc_attention_mispronunciation_amd.hip_model import HipModel
out = []
for H in (384, 256):
    geom = synth.Geometry(**dict(synth.REFERENCE, hidden=H))
    sd = synth.synth_state_dict(geom, seed=77)
    for B in (100, 512, 700, 1000):
        x, x1, _, _ = synth.synth_batch(geom, B=B, T=40, L=6, seed=B, ragged=True)
        m = HipModel(geom, sd, precision="bf16x3", taps=True)
        lp = m.forward(torch.from_numpy(x).cuda(), torch.from_numpy(x1).cuda(), sync_errors=True).cpu().numpy()
        h = hashlib.sha256(lp.tobytes())
        for n in ("rnn0", "rnn1", "rnn2", "rnn3", "text"):
            h.update(m.tap(n).cpu().numpy().tobytes())
        out.append(h.hexdigest())
print("DIGEST " + " ".join(out))
""" % ROOT
    digests = []
    for lib in (None, twin):
        env = dict(os.environ)
        if lib:
            env["MDD_LIB_PATH"] = lib
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        digests.append([l for l in r.stdout.splitlines() if l.startswith("DIGEST ")][-1])
    assert digests[0] == digests[1], (digests[0], digests[1])


@pytest.mark.parametrize("B", [512, 700])
def test_persistent_lstm_stale_panel_redo_path(B, monkeypatch):
    """The BiLSTM uses a panel requested ahead without checking it first and redoes the tile's products when the tags
    summed on the way say it was stale.  With the request placed where it normally is that never happens, so the
    diagnostic switch MDD_LSTM_EARLY moves it a whole MFMA section earlier: redos must occur, results must not move."""
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=78)
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=420, L=6, seed=B, ragged=False)
    ref = _hip().HipModel(geom, sd, precision="bf16x3").forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    monkeypatch.setenv("MDD_LSTM_EARLY", "1")
    monkeypatch.setenv("MDD_LSTM_DBG", "1")
    m = _hip().HipModel(geom, sd, precision="bf16x3")
    got = m.forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
    np.testing.assert_array_equal(got, ref)
    passes = m.tap("lstm_dbg").view(torch.int64).view(256, 6)[:, 5].cpu().numpy()
    nbt, steps = (B // 16 + 15) // 16, 420 // 4
    assert passes.min() >= nbt * (steps - 1) and passes.max() > nbt * (steps - 1), (passes.min(), passes.max(), nbt * (steps - 1))
    print("B=%d: %.2f panels fetched per (tile, step), 1.00 = no redo" % (B, passes.mean() / (nbt * (steps - 1))))


def test_decoders_edge_cases_against_oracle():
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import GreedyDecoder, BeamDecoder
    i2c = synth.phone_table_41()
    Cn, T = 45, 12
    lp = np.stack([synth.peaky_logp(T, Cn, 5, seed=s) for s in range(5)], axis=1)
    lens = [0, 1, T, T + 50, 3]                     # empty, single frame, full, longer than the tensor (clamped), short
    gd = GreedyDecoder(i2c, space_idx=-1, blank_index=0)
    ids, n = gd.decode_ids(torch.from_numpy(lp).cuda(), lens)
    ids, n = ids.cpu().numpy(), n.cpu().numpy()
    assert [ids[b, :n[b]].tolist() for b in range(5)] == oracle.greedy(lp, [min(v, T) for v in lens])
    assert gd.decode(torch.from_numpy(lp), lens)[0] == ""
    for width in (1, 10, 16, 40):                   # 40 > fast-path limit: generic kernel
        bd = BeamDecoder(i2c, beam_width=width, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=0.25)
        ids, n, st, sc = bd.decode_ids(torch.from_numpy(lp).cuda(), lens)
        want, wst, wsc = oracle.beam(lp, lens, bd.lm.dense_table(i2c, Cn), beam_width=width, alpha=0.25, return_scores=True)
        np.testing.assert_array_equal(st.cpu().numpy(), wst)
        assert wst[0] == 1                           # no frames -> IndexError in the reference
        ids, n = ids.cpu().numpy(), n.cpu().numpy()
        assert [ids[b, :n[b]].tolist() for b in range(5)] == want, width
    with pytest.raises(IndexError):
        bd.decode(torch.from_numpy(lp), lens)


def test_ctc_edge_cases_against_oracle():
    rs = np.random.Generator(np.random.PCG64(5))
    T, B, Cn, Lmax = 9, 4, 7, 4
    lp = torch.log_softmax(torch.from_numpy(rs.standard_normal((T, B, Cn)).astype(np.float32)), -1).numpy()
    tg = np.array([[1, 1, 1, 1], [2, 3, 0, 0], [4, 0, 0, 0], [5, 6, 5, 6]])
    il = np.array([9, 5, 1, 9]); tl = np.array([4, 2, 1, 4])          # repeats need blanks: row 0 is barely feasible (T = 2L+1... 9 >= 7)
    nll, grad = _hip().ctc_loss(_cuda(lp), _cuda(tg), _cuda(il), _cuda(tl))
    onll, ograd = oracle.ctc_loss(lp, tg, il, tl)
    ref = torch.nn.CTCLoss(reduction="none")(torch.from_numpy(lp), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)).numpy()
    np.testing.assert_allclose(nll.cpu().numpy(), ref, rtol=1e-5)
    np.testing.assert_allclose(nll.cpu().numpy(), onll, rtol=1e-6)
    np.testing.assert_allclose(grad.cpu().numpy(), ograd, rtol=0, atol=2e-6)
    nll_only, g = _hip().ctc_loss(_cuda(lp), _cuda(tg), _cuda(il), _cuda(tl), want_grad=False)
    assert g is None
    np.testing.assert_array_equal(nll_only.cpu().numpy(), nll.cpu().numpy())


def test_batch_evaluation_golden_and_oracle():
    """SURVEY 8(f) #2 through the C ABI (mdd_eval_batch) and its host mirror: the reference's own counts (G8), the
    helper's four return values, the exception on an empty decode, and random batches against the oracle."""
    from ctc_attention_mispronunciation_amd.steps.test_ctc_nosil import (count_batch, print_align_space_canonical_origin,
                                                                          strip_sil, MddCounts)
    g = jload("g8_eval.json")
    keys = ("total", "TA", "FR", "FA", "TRc", "TRw", "total_wer", "num_word")
    total = MddCounts()
    for b in g["batches"]:
        assert strip_sil(b["decoded"]) == b["decoded_nosil"] and strip_sil(b["canonicals"]) == b["canonicals_nosil"]
        c = count_batch(b["decoded"], b["labels"], b["canonicals"])
        assert c.as_list() == [b[k] for k in keys], b
        if b["error"] is None:
            rep = c.report()
            np.testing.assert_allclose([rep["precision"], rep["recall"], rep["F1"]], [b["precision"], b["recall"], b["f1"]], rtol=1e-12)
        else:
            with pytest.raises(ZeroDivisionError):
                c.report()
        total = total + c
    assert total.as_list() == [sum(b[k] for b in g["batches"]) for k in keys]
    for r in g["singles"]:
        a, bb, c, d = print_align_space_canonical_origin(r["s1"], r["s2"], list(r["path"]))
        assert [a, bb, c] == r["out"] and {str(k): v for k, v in d.items()} == r["d"], r
    with pytest.raises(TypeError):
        count_batch(["sil"], ["aa b"], ["aa b"])
    units = [synth.phone_table_41()[i] for i in range(3, 44)]
    rs = np.random.Generator(np.random.PCG64(5))
    for _ in range(20):
        n = int(rs.integers(1, 40))
        mk = lambda: " ".join(units[int(j)] for j in rs.integers(0, 6, size=int(rs.integers(1, 25))))  # noqa: E731
        dec, lab, can = [mk() for _ in range(n)], [mk() for _ in range(n)], [mk() for _ in range(n)]
        assert count_batch(dec, lab, can).as_list() == oracle.eval_counts(dec, lab, can)


def test_fbank_kernel_against_oracle():
    """the HIP filterbank (+ fused CMVN) against the numpy restatement of Kaldi's algorithm, on a word
    from the reference's own egs/vocabulary/single (data fixture) and on noise; then through stack/skip into the
    [T, 243] rows the model consumes.  Parity with Kaldi itself is unpinned; tolerance here is on log values."""
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.data_loader import stack_features
    wav, sr = fb.read_wav(os.path.join(GOLD, "vocabulary_single_1.wav"))
    assert sr == 16000
    stats = fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt"))
    want = oracle.fbank(wav)
    got = fb.compute_fbank_feats(wav).cpu().numpy()
    assert got.shape == want.shape == (282, 81)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-3)
    gotn = fb.compute_fbank_feats(wav, cmvn=fb.cmvn_scale_offset(stats)).cpu().numpy()
    np.testing.assert_allclose(gotn, oracle.apply_cmvn(want, stats), rtol=0, atol=2e-3)
    rs = np.random.Generator(np.random.PCG64(9))
    for n in (399, 400, 559, 560, 16000, 48017):
        x = (rs.standard_normal(n) * 3000).astype(np.float32)
        g = fb.compute_fbank_feats(x).cpu().numpy()
        w = oracle.fbank(x)
        assert g.shape == w.shape == (max(0, 1 + (n - 400) // 160) if n >= 400 else 0, 81)
        if len(w):
            np.testing.assert_allclose(g, w, rtol=0, atol=2e-3)
    stacked = stack_features(torch.from_numpy(gotn[None]).cuda()).cpu().numpy()
    np.testing.assert_array_equal(stacked[0], oracle.stack_skip(gotn))
    with pytest.raises(ValueError):
        fb.compute_fbank_feats(wav, sample_rate=8000)


def test_wav_to_diagnosis_end_to_end():
    """Config (1) without any subprocess: WAV -> fbank + CMVN (HIP) -> stack/skip -> forward -> Beam(10) (what infer.py
    runs, ctc_config.0329.yaml:86) -> alignment and diagnosis, all through the product.
    (a) on the SAME features the G9 golden was made from (oracle.fbank of the fixture WAV; Kaldi itself is absent, so the
    features are unpinned), the posteriors are within 1e-4 of the reference model's and the decoded strings, op paths,
    fault lists and score are identical to the reference's chain;
    (b) on the HIP front-end's own features (<= 7e-4 from the oracle's on log-mel values) the posteriors stay within
    2e-3 and the diagnosis is produced by the same code path."""
    from tests.helpers import chain_inputs, check_chain
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import GreedyDecoder, BeamDecoder
    from ctc_attention_mispronunciation_amd.utils.data_loader import stack_features
    from ctc_attention_mispronunciation_amd.infer_core import diagnose
    meta = [m for m in jload("g9_chain.json") if m["tag"] == "wav"][0]
    g = npz("g9_chain.npz")
    geom, sd, _, x1, frac, _ = chain_inputs(meta)
    i2c = synth.phone_table_41()
    arpa = os.path.join(GOLD, "lm_synth45.arpa")
    greedy = GreedyDecoder(i2c, space_idx=-1, blank_index=0)
    beam = BeamDecoder(i2c, beam_width=10, blank_index=0, space_idx=-1, lm_path=arpa, lm_alpha=0.0)
    for precision in ("f32", "bf16x3"):
        m = _hip().HipModel(geom, sd, precision=precision)
        logp = m.forward(_cuda(g["wav_feats"][None]), _cuda(x1), sync_errors=True)
        np.testing.assert_allclose(logp.cpu().numpy(), g["wav_logp"], rtol=0, atol=TOL)
        lens = [logp.shape[0]]
        check_chain(meta["records"], beam.decode(logp, lens), greedy.decode(logp, lens), greedy.wer,
                    lambda hyp, can: diagnose(hyp, can, greedy))
    # (b) the product's own front-end
    wav, _ = fb.read_wav(os.path.join(GOLD, "vocabulary_single_1.wav"))
    stats = fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt"))
    x = stack_features(fb.compute_fbank_feats(wav, cmvn=fb.cmvn_scale_offset(stats))[None])      # [1, T, 243], T even
    assert x.shape == (1, 142, 243)
    np.testing.assert_allclose(x.cpu().numpy()[0], g["wav_feats"], rtol=0, atol=2e-3)
    logp2 = m.forward(x, _cuda(x1), sync_errors=True)
    np.testing.assert_allclose(logp2.cpu().numpy(), g["wav_logp"], rtol=0, atol=2e-3)
    hyp = beam.decode(logp2, [logp2.shape[0]])[0]
    rep = diagnose(hyp, meta["canonical"], greedy)
    assert 0 <= rep["score"] <= 100 and len(rep["path"]) >= len(meta["canonical"].split())
    if hyp == meta["records"][0]["beam"]:
        assert rep["score"] == meta["records"][0]["beam_chain"]["score"]


@pytest.mark.parametrize("precision", ["f32", "f32x6", "bf16x3"])
def test_vocabulary_single_all_words(precision):
    """BASELINE configs[0] over ALL 20 words of egs/vocabulary/single (G12, made by the reference's own chain): N.txt -> the offline
    lexicon (dict/phonetic_dict.py: CMU dictionary lookup + the stress post-processing of AA/infer.py:543-548) -> canonical ids,
    identical to the reference's lookup, the two words the dictionary lacks included (no canonical: the reference would ask g2p_en /
    espeak, absent offline); N.wav -> features -> HIP forward -> Beam(10) (what infer.py runs) and Greedy -> wer -> alignment ->
    fault lists -> score.
    (a) on the features the golden was made from (oracle.fbank + CMVN + stack/skip of the WAV, recomputed here: Kaldi itself is absent,
    so feature parity is unpinned) the posteriors are within 1e-4 of the reference model's and every decoded string, op path, fault
    list and score is identical to the reference's chain -- all 18 words with a canonical;
    (b) WAV -> mdd_fbank (the product's own front-end, <= 7e-4 from the oracle's log-mel values) -> the same chain: posteriors still
    within 1e-4 (measured 2.4e-6 in fp32 mode, 8.1e-6 in the split-bf16 variant) and the whole diagnosis identical for all 18 words."""
    from tests.helpers import check_chain, record_margin
    from oracle import oracle as orc
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import GreedyDecoder, BeamDecoder
    from ctc_attention_mispronunciation_amd.utils.data_loader import stack_features
    from ctc_attention_mispronunciation_amd.infer_core import diagnose
    from ctc_attention_mispronunciation_amd.dict.phonetic_dict import Phonetic
    meta, g = jload("g12_words.json"), npz("g12_words.npz")
    assert [r["i"] for r in meta] == list(range(1, 21))
    lex = Phonetic(os.path.join(GOLD, "cmudict_subset.dict"))
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=11)
    i2c = synth.phone_table_41()
    c2i = {v: k for k, v in i2c.items()}
    greedy = GreedyDecoder(i2c, space_idx=-1, blank_index=0)
    beam = BeamDecoder(i2c, beam_width=10, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=0.0)
    stats = fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt"))
    ostats = orc.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt"))
    m = _hip().HipModel(geom, sd, precision=precision)
    worst_a = worst_b = 0.0
    same_b = chained = 0
    for rec in meta:
        word = open(os.path.join(GOLD, "vocabulary_single", "%d.txt" % rec["i"])).read().strip()
        assert word == rec["word"]
        cmu = lex.cmu_dict(word)
        assert cmu == rec["cmu"], (word, cmu, rec["cmu"])
        if rec["canonical"] is None:
            assert cmu is None
            continue
        canon = Phonetic.phones_for_model(cmu)
        assert canon == rec["canonical"]
        x1 = _cuda(np.array([[c2i[p] for p in canon.split()]], dtype=np.int64))
        wav, rate = fb.read_wav(os.path.join(GOLD, "vocabulary_single", "%d.wav" % rec["i"]))
        assert rate == 16000 and wav.size == rec["samples"]
        # (a) the golden's own features
        feats = orc.stack_skip(orc.apply_cmvn(orc.fbank(wav.astype(np.float32)), ostats))
        assert feats.shape[0] == rec["T"]
        logp = m.forward(_cuda(feats[None]), x1, sync_errors=True)
        ref = g["logp%d" % rec["i"]]
        worst_a = max(worst_a, float(np.abs(logp.cpu().numpy() - ref).max()))
        np.testing.assert_allclose(logp.cpu().numpy(), ref, rtol=0, atol=TOL, err_msg=word)
        lens = [logp.shape[0]]
        check_chain(rec["records"], beam.decode(logp, lens), greedy.decode(logp, lens), greedy.wer, lambda hyp, can: diagnose(hyp, can, greedy))
        chained += 1
        # (b) the product's own front-end
        x = stack_features(fb.compute_fbank_feats(wav, cmvn=fb.cmvn_scale_offset(stats))[None])
        assert x.shape == (1, rec["T"], 243)
        logp2 = m.forward(x, x1, sync_errors=True)
        worst_b = max(worst_b, float(np.abs(logp2.cpu().numpy() - ref).max()))
        np.testing.assert_allclose(logp2.cpu().numpy(), ref, rtol=0, atol=TOL, err_msg=word)
        hb, hg = beam.decode(logp2, lens), greedy.decode(logp2, lens)
        if hb[0] == rec["records"][0]["beam"] and hg[0] == rec["records"][0]["greedy"]:
            check_chain(rec["records"], hb, hg, greedy.wer, lambda hyp, can: diagnose(hyp, can, greedy))
            same_b += 1
        else:
            rep = diagnose(hb[0], canon, greedy)
            assert 0 <= len(rep["path"]) and isinstance(rep["score"], int)
    print("vocabulary/single, %s: %d words chained; max|logp - reference| %.2e on the golden's features, %.2e from the WAV through mdd_fbank; "
          "%d / %d words decode to the reference's strings from the WAV" % (precision, chained, worst_a, worst_b, same_b, chained))
    record_margin("vocabulary_single_%s_logp_same_features" % precision, worst_a, TOL)
    record_margin("vocabulary_single_%s_logp_from_wav" % precision, worst_b, TOL)
    assert chained == 18 and same_b == 18


@pytest.mark.parametrize("precision", ["f32", "f32x6", "bf16x3"])
@pytest.mark.parametrize("idx", [0, 1, 2])
def test_benchmarked_length_golden_and_chain(idx, precision):
    """G9 (made by the reference's own Python): log-probs at the benchmarked length T'=250 (ragged lengths, ragged L,
    H=384 and H=256) within 1e-4 in BOTH arithmetic modes; then HIP forward -> product BeamDecoder(10) / GreedyDecoder
    -> Decoder.wer -> infer_core: strings, op paths, fault lists and scores IDENTICAL to the reference's chain."""
    from tests.helpers import chain_inputs, check_chain
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import GreedyDecoder, BeamDecoder
    from ctc_attention_mispronunciation_amd.utils.data_loader import frames_from_fraction
    from ctc_attention_mispronunciation_amd.infer_core import diagnose
    meta = jload("g9_chain.json")[idx]
    ref = npz("g9_chain.npz")[meta["tag"] + "_logp"]
    geom, sd, x, x1, frac, _ = chain_inputs(meta)
    m = _hip().HipModel(geom, sd, precision=precision)
    assert m.precision == precision
    logp = m.forward(_cuda(x), _cuda(x1), sync_errors=True)
    err = np.abs(logp.cpu().numpy() - ref).max()
    print("%s %s: max|logp - reference| at T'=%d = %.2e" % (meta["tag"], precision, ref.shape[0], err))
    from tests.helpers import record_margin
    record_margin("g9_%s_%s_logp" % (meta["tag"], precision), err, TOL)
    np.testing.assert_allclose(logp.cpu().numpy(), ref, rtol=0, atol=TOL)
    lens = frames_from_fraction(torch.from_numpy(frac), logp.shape[0]).tolist()
    assert lens == [r["len"] for r in meta["records"]]
    i2c = synth.phone_table_41()
    greedy = GreedyDecoder(i2c, space_idx=-1, blank_index=0)
    beam = BeamDecoder(i2c, beam_width=10, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=0.0)
    check_chain(meta["records"], beam.decode(logp, lens), greedy.decode(logp, lens), greedy.wer,
                lambda hyp, can: diagnose(hyp, can, greedy))


@pytest.mark.parametrize("H", [384, 256])
def test_split_bf16_against_exact_fp32_at_bench_size(H):
    """The benchmarked arithmetic against the exact-fp32 mode of the same library at the benchmarked size (B=64 ragged,
    T'=250, L=40): max|dlogp| inside the 1e-4 tolerance, and the decoded beam / greedy ids of all 64 utterances identical
    (the recurrent state is carried as bf16 hi+lo, ~16 bits, through 250 steps x 4 layers)."""
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import GreedyDecoder, BeamDecoder
    from ctc_attention_mispronunciation_amd.utils.data_loader import frames_from_fraction
    geom = synth.Geometry(**dict(synth.REFERENCE, hidden=H))
    sd = synth.synth_state_dict(geom, seed=1234)
    x, x1, frac, _ = synth.synth_batch(geom, B=64, T=500, L=40, seed=1234, ragged=True)
    out = {}
    for precision in ("f32", "bf16x3"):
        out[precision] = _hip().HipModel(geom, sd, precision=precision).forward(_cuda(x), _cuda(x1), sync_errors=True)
    d = (out["f32"] - out["bf16x3"]).abs().max().item()
    print("H=%d B=64 T'=250: max|logp(bf16x3) - logp(f32)| = %.2e" % (H, d))
    assert d < TOL
    i2c = synth.phone_table_41()
    lens = frames_from_fraction(torch.from_numpy(frac), 250).tolist()
    greedy = GreedyDecoder(i2c, space_idx=-1, blank_index=0)
    beam = BeamDecoder(i2c, beam_width=10, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=0.0)
    assert greedy.decode(out["f32"], lens) == greedy.decode(out["bf16x3"], lens)
    a, b = beam.decode(out["f32"], lens), beam.decode(out["bf16x3"], lens)
    assert a == b, [i for i in range(64) if a[i] != b[i]]


def test_error_against_fp64_beside_aten_fp32():
    """Whose fp32 is closer to the truth?  One benchmark-sized batch (B = 64 ragged, T' = 250, L = 40, H = 384) through (1) the
    restatement of the reference on ATen CPU ops in DOUBLE (oracle/ref_port.forward, pinned by the goldens) -- the yardstick --,
    (2) the same graph in float32 = what the reference itself computes, (3) this library's reference-width mode (exact fp32 MFMA)
    and (4) its flagged split-bf16 variant.  Measured (kept in gpurun_out/margins.json): ATen fp32 max 2.2e-6 / mean 3.3e-7, the
    reference-width mode max 4.0e-6 / mean 4.7e-7 -- the same arithmetic (exact fp32 products, fp32 accumulate) in another order: an
    MFMA GEMM is ONE accumulation chain per output over K = 1952 / 768, ATen's CPU kernels keep 8-16 partial sums -- the variant max
    1.0e-5 / mean 1.7e-6.  Asserted: the reference-width mode within 2x of ATen's own distance (max and mean), the variant inside the
    1e-4 budget."""
    from oracle import ref_port
    from tests.helpers import record_margin
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=1234)
    x, x1, frac, _ = synth.synth_batch(geom, B=64, T=500, L=40, seed=1234, ragged=True)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    ref64 = ref_port.forward(sd, x, x1, dtype=torch.float64).numpy()
    aten32 = ref_port.forward(sd, x, x1).numpy().astype(np.float64)
    got = {p: _hip().HipModel(geom, sd, precision=p).forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy().astype(np.float64)
           for p in ("f32", "bf16x3", "f32x6")}
    lens = (torch.from_numpy(frac) * 250).long().numpy()
    live = np.zeros(ref64.shape[:2], dtype=bool)
    for b, n in enumerate(lens):
        live[:n, b] = True                                       # frames the decoders read (padded frames are computed too, by both sides)
    stats = {}
    for name, v in (("aten_f32", aten32), ("hip_f32", got["f32"]), ("hip_f32x6", got["f32x6"]), ("hip_bf16x3", got["bf16x3"])):
        d = np.abs(v - ref64)
        stats[name] = (float(d.max()), float(d.mean()), float(d[live].max()))
        record_margin("fp64_distance_%s_max" % name, stats[name][0], TOL)
        record_margin("fp64_distance_%s_mean" % name, stats[name][1])
    print("distance to the float64 evaluation, B=64 x T'=250: " + "; ".join("%s max %.2e mean %.2e" % (k, v[0], v[1]) for k, v in stats.items()))
    assert stats["hip_f32"][0] <= 2.0 * stats["aten_f32"][0] and stats["hip_f32"][1] <= 2.0 * stats["aten_f32"][1]
    # f32x6 (three bf16 planes per operand in the input projections): it must be AT LEAST as close to float64 as ATen's fp32 is
    assert stats["hip_f32x6"][1] <= stats["aten_f32"][1] and stats["hip_f32x6"][0] <= 1.25 * stats["aten_f32"][0], stats
    assert stats["hip_bf16x3"][0] < TOL


@pytest.mark.parametrize("T_raw", [1000, 997, 250, 7])
@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_forward_raw_equals_stack_then_forward(T_raw, precision):
    """mdd_forward_raw (stack/skip folded into the fused front-end's tile load, or an internal stacked copy in the exact
    mode) gives the bits of stack_features followed by forward -- odd lengths, the repeated last frame and the zero row
    that pads to an even count included."""
    from ctc_attention_mispronunciation_amd.utils.data_loader import stack_features
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=5)
    raw = torch.from_numpy(synth.synth_raw_features(3, T_raw, 81, seed=T_raw)).cuda()
    _, x1, _, _ = synth.synth_batch(geom, B=3, T=max(2, T_raw // 2 * 2), L=5, seed=1, ragged=False)
    x1 = _cuda(x1)
    m = _hip().HipModel(geom, sd, precision=precision)
    want = m.forward(stack_features(raw), x1, sync_errors=True).cpu().numpy()
    got = m.forward_raw(raw, x1, sync_errors=True).cpu().numpy()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("M,N,K", [(256, 512, 32), (1024, 512, 64), (4096, 3072, 768), (4100, 3072, 1952), (16000, 3072, 768), (1300, 800, 96)])
def test_gemm_8phase_race_screen(M, N, K):
    """The 8-phase projection GEMM (two wave groups a barrier apart, LDS-DMA in flight across raw barriers, counted
    vmcnt) performs the same arithmetic per C element as the single-barrier kernel: pseudo-random operands through
    both, the 8-phase one 12 times per shape, every C word compared -- including one-K-tile, two-K-tile, ragged-M and
    ragged-N shapes.  A synchronisation slip would show as a mismatch in some repetition."""
    import ctypes as C
    from ctypes import c_int, c_uint
    from ctc_attention_mispronunciation_amd import _lib
    L = _lib.lib()
    torch.zeros(1).cuda()
    bad = c_uint(12345)
    for seed in (1, 2):
        rc = L.mdd_diag_gemm_ph8(c_int(M), c_int(N), c_int(K), c_int(12), c_uint(seed), C.byref(bad), None)
        assert rc == 0, L.mdd_last_error().decode()
        assert bad.value == 0, (M, N, K, seed, bad.value)



def test_two_handles_two_streams_share_one_device():
    """Two HipModels, two host threads, two HIP streams, one device, B=64 at full length: a persistent BiLSTM layer needs
    every CU, so the library orders such forwards behind one another per device (api.hip DeviceGate) instead of letting
    their workgroups starve each other until the wall-clock abort.  Both must return the single-handle bits, with no
    MDD_ERR_HIP from mdd_sync."""
    import threading
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=1234)
    batches = []
    for k in range(2):
        x, x1, _, _ = synth.synth_batch(geom, B=64, T=500, L=40, seed=50 + k, ragged=True)
        batches.append((_cuda(x), _cuda(x1)))
    solo = _hip().HipModel(geom, sd, precision="bf16x3")
    want = [solo.forward(x, x1, sync_errors=True).cpu().numpy() for x, x1 in batches]
    models = [_hip().HipModel(geom, sd, precision="bf16x3") for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    got, errs = [[], []], []
    start = threading.Barrier(2)

    def worker(k):
        try:
            torch.cuda.set_device(0)
            x, x1 = batches[k]
            with torch.cuda.stream(streams[k]):
                start.wait()
                for _ in range(6):                       # several forwards in flight per stream, interleaved with the other's
                    got[k].append(models[k].forward(x, x1, out=None))
                models[k].forward(x, x1, sync_errors=True)
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))
    torch.cuda.synchronize()
    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    torch.cuda.synchronize()
    assert not errs, errs
    for k in range(2):
        for lp in got[k]:
            np.testing.assert_array_equal(lp.cpu().numpy(), want[k])


@pytest.mark.parametrize("what", ["ids", "posteriors"])
def test_bench_two_ranks_rehearsal(what):
    """The N>1 path of bench.py, rehearsed as 2 ranks on the ONE GPU of this box: launched exactly as the driver launches
    it (torch.distributed.run), gloo instead of RCCL (two ranks cannot form an RCCL ring on one device) and the per-step
    BiLSTM kernels (a persistent layer needs every CU of the device; the per-device gate is per process).  Checks the
    contract line, n_gpus, and that each rank's slice of the exchanged results (decoded ids by default, posteriors on request) is
    its own output.  (Where the exchange sits relative to the next forward: test_bench_exchange_runs_beside_the_next_forward.)"""
    import socket
    import subprocess
    import sys
    from tests.helpers import ROOT
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MDD_DIST_BACKEND="gloo", MDD_LSTM="step", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--fuse", "1",
           "--full", "--no-cpu-baseline", "--no-roofline", "--gather", what]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 4 and out["scaling"] == "weak" and out["value"] > 0
    assert out["config"]["global_batch"] == 128 and ("all-gather of %s" % what) in out["config"]["parallelism"]
    assert out["gather_verified"] is True
    assert out["gather_timing"]["what"] == what


def test_bench_exchange_runs_beside_the_next_forward():
    """Stream structure of the N>1 path, by device timestamps: the result exchange of pass i sits on its own stream and depends only
    on its own pass, so the forward of pass i+1 starts as soon as the forward of pass i ends -- however long the exchange takes.
    One process with a one-rank RCCL group (MDD_FORCE_DIST=1: two ranks sharing this box's single GPU would time-slice it and
    blur the timestamps); the exchange is stretched by a spinning kernel in front of the collective (MDD_BENCH_GATHER_DELAY_MS),
    which with the collective on the forward stream -- round 2's arrangement -- would appear in the gap one for one."""
    import subprocess
    import sys
    from tests.helpers import ROOT
    env = dict(os.environ, MDD_FORCE_DIST="1", MDD_LSTM="step", MDD_BENCH_GATHER_DELAY_MS="12", HSA_ENABLE_IPC_MODE_LEGACY="0",
               MASTER_ADDR="127.0.0.1", MASTER_PORT="29571", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--fuse", "1",
           "--full", "--no-cpu-baseline", "--no-roofline", "--no-variants", "--gather", "posteriors"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    gt = out["gather_timing"]
    print("exchange beside the next forward: %s; ms_per_step %.2f" % (gt, out["ms_per_step"]))
    assert out["gather_verified"] is True and gt["what"] == "posteriors"
    assert gt["gather_ms_median"] > 4.0                          # the stretched exchange
    assert gt["forward_stream_gap_ms_median"] < 0.25 * gt["gather_ms_median"] and gt["forward_stream_gap_ms_median"] < 1.0


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A plain bench.py run (no --full): the headline line with exactly --steps timed steps and none of --full's extras; with
    --dump-outputs, the last timed pass's results as float arrays.  --steps 3 --fuse 2 makes the passes [2 batches, 1 batch], so the
    last pass is the first 64 seeded utterances alone: its log-probs equal a lone forward_raw of them, its decoded ids stop at
    their lengths, and its edit distances to the 40 canonical phonemes lie within the bounds their lengths allow."""
    import subprocess
    import sys
    from tests.helpers import ROOT
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--fuse", "2",
           "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["higher_is_better"] is True
    assert out["unit"] == "phoneme-frames/s" and out["dtype"].startswith("f32")
    assert out["roofline"] is None and out["cpu_baseline"] is None and out["accuracy"] is None and out["variants"] is None
    got = {p.stem: np.load(p) for p in dump.glob("*.npy")}
    assert set(got) == {"log_probs", "decoded_ids", "decoded_len", "beam_status", "beam_score", "edit_distance", "utterance"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(p.stat().st_size for p in dump.glob("*.npy")) <= 64 << 20
    B, Tp = 64, 250
    assert got["log_probs"].shape == (Tp, B, 45) and got["decoded_ids"].shape == (B, Tp)
    np.testing.assert_array_equal(got["utterance"], np.arange(B))
    n, ids, d = got["decoded_len"].astype(int), got["decoded_ids"], got["edit_distance"].astype(int)
    assert all(((ids[b, :n[b]] > 0) & (ids[b, :n[b]] < 45)).all() and (ids[b, n[b]:] == -1).all() for b in range(B))
    assert all(abs(n[b] - 40) <= d[b] <= max(n[b], 40) if n[b] else d[b] == -1 for b in range(B))     # canonical length 40
    geom = synth.Geometry(feat=243, hidden=384, layers=4, num_class=45)
    raw = synth.synth_raw_features(128, 1000, 81, seed=1234)[:B]
    x1 = synth.synth_batch(geom, B=128, T=500, L=40, seed=1234, ragged=False)[1][:B]
    m = HipModel(geom, synth.synth_state_dict(geom, seed=1234), device=0)
    want = m.forward_raw(_cuda(raw), _cuda(x1), sync_errors=True).cpu().numpy()
    m.close()
    np.testing.assert_allclose(got["log_probs"], want, rtol=0, atol=1e-6)


@pytest.mark.parametrize("L,T,B", [(40, 250, 8), (100, 300, 3), (200, 420, 2), (63, 130, 4), (64, 130, 4), (1, 5, 3)])
def test_ctc_wave_kernel_label_widths_against_oracle(L, T, B, monkeypatch):
    """The wavefront lattice kernel at 1, 2 and 4 labels per lane (Lmax <= 63 / 127 / 255), ragged input and label lengths,
    repeated labels: against the fp64 oracle, against the generic (one-thread-per-state) kernel, and bit-identical from run
    to run (the per-class sums use no atomics)."""
    rs = np.random.Generator(np.random.PCG64(L * 1000 + T))
    Cn = 45
    lp = torch.log_softmax(torch.from_numpy((rs.standard_normal((T, B, Cn)) * 2.0).astype(np.float32)), -1).numpy()
    tg = rs.integers(1, Cn, size=(B, L))
    if L > 2:
        tg[:, 1] = tg[:, 0]                                   # repeats: a blank is forced between them
    tl = rs.integers(max(1, L // 2), L + 1, size=B); tl[0] = L
    il = np.array([min(T, max(int(rs.integers(T // 2, T + 1)), 2 * int(tl[b]) + 2)) for b in range(B)]); il[0] = T
    nll, grad = _hip().ctc_loss(_cuda(lp), _cuda(tg), _cuda(il), _cuda(tl))
    onll, ograd = oracle.ctc_loss(lp, tg, il, tl)
    assert np.isfinite(onll).all()
    np.testing.assert_allclose(nll.cpu().numpy(), onll, rtol=1e-6)
    np.testing.assert_allclose(grad.cpu().numpy(), ograd, rtol=0, atol=5e-6)
    nll2, grad2 = _hip().ctc_loss(_cuda(lp), _cuda(tg), _cuda(il), _cuda(tl))
    assert torch.equal(nll, nll2) and torch.equal(grad, grad2)
    monkeypatch.setenv("MDD_CTC", "generic")
    nll3, grad3 = _hip().ctc_loss(_cuda(lp), _cuda(tg), _cuda(il), _cuda(tl))
    np.testing.assert_allclose(nll3.cpu().numpy(), onll, rtol=1e-6)
    np.testing.assert_allclose(grad3.cpu().numpy(), ograd, rtol=0, atol=2e-6)


def test_ctc_bad_labels_infeasible_rows_and_workspace_contract():
    import ctypes as C
    from ctc_attention_mispronunciation_amd import _lib
    rs = np.random.Generator(np.random.PCG64(3))
    T, B, Cn, L = 20, 4, 9, 5
    lp = torch.log_softmax(torch.from_numpy(rs.standard_normal((T, B, Cn)).astype(np.float32)), -1).numpy()
    tg = rs.integers(1, Cn, size=(B, L))
    tg[1, 2] = Cn            # label outside [0, C): NaN for that utterance, zero gradient rows, nothing read out of bounds
    tg[2, 0] = -3
    il = np.array([T, T, T, 3]); tl = np.array([L, L, L, L])          # row 3: 5 labels cannot fit 3 frames -> +inf (reference: inf)
    nll, grad = _hip().ctc_loss(_cuda(lp), _cuda(tg), _cuda(il), _cuda(tl))
    nll, grad = nll.cpu().numpy(), grad.cpu().numpy()
    assert np.isfinite(nll[0]) and np.isnan(nll[1]) and np.isnan(nll[2]) and np.isposinf(nll[3])
    assert not grad[:, 1].any() and not grad[:, 2].any() and not grad[3:, 3].any()
    ref = torch.nn.CTCLoss(reduction="none")(torch.from_numpy(lp), torch.from_numpy(np.clip(tg, 1, Cn - 1)), torch.from_numpy(il), torch.from_numpy(tl)).numpy()
    np.testing.assert_allclose(nll[0], ref[0], rtol=1e-5)
    assert np.isposinf(ref[3])
    # a caller workspace that is too small is refused, not overrun
    L_ = _lib.lib()
    need = L_.mdd_ctc_workspace_bytes(T, B, Cn, L, 1)
    assert need > 0 and L_.mdd_ctc_workspace_bytes(T, B, Cn, L, 0) == 0
    small = torch.empty(need // 8 - 1, dtype=torch.float64, device="cuda")
    lpd, tgd, ild, tld = _cuda(lp), _cuda(np.clip(tg, 1, Cn - 1)), _cuda(il), _cuda(tl)
    out_n = torch.empty(B, device="cuda"); out_g = torch.empty((T, B, Cn), device="cuda")
    args = [C.c_void_p(lpd.data_ptr()), T, B, Cn, C.c_void_p(tgd.data_ptr()), L, C.c_void_p(ild.data_ptr()), C.c_void_p(tld.data_ptr()), 0,
            C.c_void_p(out_n.data_ptr()), C.c_void_p(out_g.data_ptr())]
    assert L_.mdd_ctc_loss(*args, C.c_void_p(small.data_ptr()), small.numel() * 8, None) == -1
    assert L_.mdd_ctc_loss(*args, None, 0, None) == 0                  # no workspace: the library allocates stream-ordered
    torch.cuda.synchronize()
    np.testing.assert_allclose(out_n.cpu().numpy()[:3], ref[:3], rtol=1e-5)


# ---------------------------------------------------------------------------- training step (BASELINE config 5)
def _train_model(geom, sd):
    import torch.nn as nn
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    model = CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=0.2)
    if geom.emb_rows != 44 or geom.emb_dim != 512:          # tiny geometry (as oracle/gen_golden.py builds the reference)
        model.embeds = nn.Embedding(geom.emb_rows, geom.emb_dim)
        model.lstm_embeds = nn.LSTM(geom.emb_dim, geom.hidden, batch_first=True, bidirectional=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return model.cuda().train()


def _check_grads(model, want, tol_rel=1e-4, sampled=None):
    for k, p_ in model.named_parameters():
        assert p_.grad is not None, k
        got = p_.grad.cpu().numpy()
        if k.endswith("conv.bias"):
            # A bias in front of a batch-statistics BatchNorm has gradient EXACTLY zero (the normalisation removes any constant);
            # what either side holds is the rounding residue of sums over 1e5..1e6 terms, so only its smallness is comparable.
            assert float(np.abs(got).max()) < 1e-3, (k, float(np.abs(got).max()))
            continue
        if sampled is not None and k in sampled:
            idx_, val, absmax = sampled[k]
            np.testing.assert_allclose(got.ravel()[idx_], val, rtol=0, atol=tol_rel * max(1.0, absmax), err_msg=k)
        else:
            w_ = want[k]
            np.testing.assert_allclose(got, w_, rtol=0, atol=tol_rel * max(1.0, float(np.abs(w_).max())), err_msg=k)


@pytest.mark.parametrize("idx", [0, 1, 2])
def test_train_step_reference_goldens(idx):
    """G11 (the reference model's own train-mode step; tiny geometry, reference geometry at T' = 8, and reference geometry at T' = 80
    with ragged input / label lengths): the drop-in CTC_Model in train mode -- BatchNorm on batch statistics,
    the reference's dropout masks handed in -- then the product CTCLoss(sum)/B and loss.backward(): log-probs within 1e-4,
    loss, EVERY parameter gradient within 1e-4 of its scale, running statistics and num_batches_tracked updated as nn.BatchNorm does."""
    from ctc_attention_mispronunciation_amd.train import CTCLoss
    meta = jload("g11_train.json")[idx]
    g = npz("g11_train.npz")
    tag = meta["tag"]
    geom = synth.Geometry(**meta["geom"])
    sd, x, x1, masks, tg, il, tl = synth.train_case(geom, meta["seed"], meta["B"], meta["T"], meta["L"], meta["Lt"])
    model = _train_model(geom, sd)
    model._dropout_masks = [torch.from_numpy(m) for m in masks]
    out = model(_cuda(x), _cuda(x1))
    assert out.requires_grad and out.shape == g[tag + "_logp"].shape
    np.testing.assert_allclose(out.detach().cpu().numpy(), g[tag + "_logp"], rtol=0, atol=TOL)
    loss = CTCLoss(reduction="sum")(out, torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)) / meta["B"]    # train_ctc.py:72-74
    assert abs(float(loss.detach()) - meta["loss"]) <= 1e-5 * abs(meta["loss"])
    loss.backward()
    full = {k[len(tag) + 6:]: g[k] for k in g.files if k.startswith(tag + "_grad_")}
    sampled = {k[len(tag) + 6:]: (g[k], g[k.replace("_gidx_", "_gval_")], meta["tensors"][k[len(tag) + 6:]]["absmax"]) for k in g.files if k.startswith(tag + "_gidx_")}
    # T' = 80: golden and product are both fp32 evaluations of BPTT over 80 steps (each ~5e-5 of scale away from the exact value, see
    # test_train_step_split_bf16_variant); one element of one BatchNorm gradient was measured 1.1e-4 of scale apart: bound 2e-4 there
    _check_grads(model, full, sampled=sampled, tol_rel=2e-4 if tag == "long" else 1e-4)
    for k, info in meta["tensors"].items():
        if k.endswith("conv.bias"):
            continue                                        # exactly-zero gradients: rounding residue on both sides (see _check_grads)
        gn = float(dict(model.named_parameters())[k].grad.double().norm())
        assert abs(gn - info["norm"]) <= 1e-3 * max(info["norm"], 1e-2), (k, gn, info["norm"])
    for k, b_ in model.named_buffers():
        if "running_" in k:
            np.testing.assert_allclose(b_.cpu().numpy(), g["%s_run_%s" % (tag, k)], rtol=0, atol=1e-5, err_msg=k)
        elif k.endswith("num_batches_tracked"):
            assert int(b_) == 8                             # synth writes 7


@pytest.mark.parametrize("H,B,T,L", [(384, 3, 24, 6), (256, 5, 40, 9)])
def test_train_step_against_torch_restatement(H, B, T, L):
    """Shapes without a golden: every tensor in full against oracle/ref_port.train_step (torch autograd on ATen CPU ops, pinned
    to the reference by G11) -- ragged lengths, batch sizes that are not tile multiples, H=384 and H=256."""
    from oracle import ref_port
    from ctc_attention_mispronunciation_amd.train import CTCLoss
    geom = synth.Geometry(**dict(synth.REFERENCE, hidden=H))
    sd, x, x1, masks, tg, il, tl = synth.train_case(geom, 100 + H, B, T, L, 4)
    logp, loss, grads, run = ref_port.train_step(sd, x, x1, masks, tg, il, tl, 0.2)
    model = _train_model(geom, sd)
    model._dropout_masks = [torch.from_numpy(m) for m in masks]
    out = model(_cuda(x), _cuda(x1))
    np.testing.assert_allclose(out.detach().cpu().numpy(), logp, rtol=0, atol=TOL)
    l2 = CTCLoss(reduction="sum")(out, torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)) / B
    assert abs(float(l2) - loss) <= 1e-5 * abs(loss)
    l2.backward()
    _check_grads(model, grads)
    for k, b_ in model.named_buffers():
        if "running_" in k:
            np.testing.assert_allclose(b_.cpu().numpy(), run[k], rtol=0, atol=1e-5, err_msg=k)


@pytest.mark.parametrize("H,B,T,L", [(384, 32, 160, 12), (256, 272, 16, 5), (256, 100, 24, 5), (384, 7, 40, 6), (256, 2, 4, 1)])
def test_train_step_split_bf16_variant(H, B, T, L):
    """The flagged variant of the training step (model.train_precision = "bf16x3": input projections, dX and dW_ih through the
    split-bf16 x3 matrix-core GEMM, the weight gradients with the row axis cut into partial products, the forward recurrences in the
    persistent layer kernel with h carried as bf16 hi/lo, the backward recurrences in the persistent BPTT kernel with the gate gradients
    travelling as bf16 hi/lo) at sizes where every one of those paths is taken (B=32, T=160: 2560 rows, one batch tile per team;
    B=272, H=256: two tiles per team forward, per-step backward; B=100 and B=7: ragged team rows), beside the exact mode, both against the restatement run in DOUBLE (at this size
    torch's own fp32 evaluation is 5e-5..9e-5 of scale away from double, so it is no yardstick).
    Exact mode: log-probs 1e-4, every gradient outside the CNN within 2e-5 of its scale (measured 7e-6).
    Variant (operands carry 16 mantissa bits): log-probs 5e-4 (logits of magnitude ~16 after four layers), gradients 2e-4 of scale.
    The CNN's gradients (conv.*) are sums over 2e7 ReLU gates, a handful of which sit within one rounding of zero: one gate flipping
    moves those sums by 2e-4..1e-3 of scale (the restatement's own fp32 result moves by 1.7e-4 under a 1-ulp change of the input,
    this path's by 2.4e-4), so for them the bound is 3e-3 in both modes.  The two modes must not be bit-identical."""
    from oracle import ref_port
    from ctc_attention_mispronunciation_amd.train import CTCLoss
    geom = synth.Geometry(**dict(synth.REFERENCE, hidden=H))
    sd, x, x1, masks, tg, il, tl = synth.train_case(geom, 77, B, T, L, max(1, min(6, T // 4)))
    logp, loss, grads, run = ref_port.train_step(sd, x, x1, masks, tg, il, tl, 0.2, dtype=torch.float64)
    got = {}
    tiny = B * T < 64     # BatchNorm over four rows: the statistics themselves are ill-conditioned in fp32; the case is there for T' = 1 / L = 1
    for mode, tol_logp, tol_loss, tol_grad in (("bf16x3", 5e-4, 1e-4, 2e-4), ("f32", TOL, 1e-5, 2e-4 if tiny else 2e-5)):
        model = _train_model(geom, sd)
        model.train_precision = mode
        model._dropout_masks = [torch.from_numpy(m) for m in masks]
        out = model(_cuda(x), _cuda(x1))
        print(mode, "max |dlogp|", float(np.abs(out.detach().cpu().numpy() - logp).max()))
        np.testing.assert_allclose(out.detach().cpu().numpy(), logp, rtol=0, atol=tol_logp, err_msg=mode)
        l2 = CTCLoss(reduction="sum")(out, torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)) / B
        assert abs(float(l2.detach()) - loss) <= tol_loss * abs(loss), mode
        l2.backward()
        errs = sorted(((float(np.abs(p_.grad.cpu().numpy() - grads[k]).max()) / max(1.0, float(np.abs(grads[k]).max())), k)
                       for k, p_ in model.named_parameters() if not k.endswith("conv.bias")), reverse=True)
        print(mode, "grad err / scale, largest:", [(k, "%.1e" % e) for e, k in errs[:6]])
        for e, k in errs:
            assert e <= (3e-3 if k.startswith("conv.") else tol_grad), (mode, k, e)
        got[mode] = {k: p_.grad.clone() for k, p_ in model.named_parameters()}
    k = "rnns.1.rnn.weight_ih_l0"
    assert not torch.equal(got["f32"][k], got["bf16x3"][k])


@pytest.mark.parametrize("H", [384])
def test_train_step_at_the_benchmarked_shape(H):
    """bench.py's train32 shape -- B = 32 utterances of 10 s (T = 500 stacked frames, T' = 250), L = 40, 20..40 labels -- in both
    arithmetic modes against the restatement run in DOUBLE (oracle/ref_port.train_step, pinned to the reference by G11): log-probs,
    loss and every parameter gradient.  This is where the persistent forward / BPTT kernels of the variant run 250 steps and the
    weight-gradient contractions run over 8 000 rows.  Bounds as in test_train_step_split_bf16_variant (exact mode: log-probs 1e-4,
    gradients 2e-5 of scale outside the CNN; variant: 5e-4 and 2e-4; conv.* 3e-3 in both, ReLU gates within one rounding of zero);
    the measured distances are kept in gpurun_out/margins.json."""
    from oracle import ref_port
    from tests.helpers import record_margin
    from ctc_attention_mispronunciation_amd.train import CTCLoss
    geom = synth.Geometry(**dict(synth.REFERENCE, hidden=H))
    B, T, L = 32, 500, 40
    sd, x, x1, masks, tg, il, tl = synth.train_case(geom, 177, B, T, L, 40)
    tl = np.maximum(tl, 20); tg = tg.copy()
    rs = np.random.Generator(np.random.PCG64(9))
    for b in range(B):
        tg[b, :tl[b]] = rs.integers(1, geom.num_class, size=tl[b])
        tg[b, tl[b]:] = 0
    il = np.minimum(np.maximum(il, 2 * tl + 1), T // 2)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    logp, loss, grads, run = ref_port.train_step(sd, x, x1, masks, tg, il, tl, 0.2, dtype=torch.float64)
    for mode, tol_logp, tol_loss, tol_grad in (("f32", TOL, 1e-5, 2e-5), ("bf16x3", 5e-4, 1e-4, 2e-4)):
        model = _train_model(geom, sd)
        model.train_precision = mode
        model._dropout_masks = [torch.from_numpy(m) for m in masks]
        out = model(_cuda(x), _cuda(x1))
        dl = float(np.abs(out.detach().cpu().numpy() - logp).max())
        l2 = CTCLoss(reduction="sum")(out, torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)) / B
        dloss = abs(float(l2.detach()) - loss) / abs(loss)
        l2.backward()
        errs = sorted(((float(np.abs(p_.grad.cpu().numpy() - grads[k]).max()) / max(1.0, float(np.abs(grads[k]).max())), k)
                       for k, p_ in model.named_parameters() if not k.endswith("conv.bias")), reverse=True)
        worst_rest = max(e for e, k in errs if not k.startswith("conv."))
        worst_conv = max(e for e, k in errs if k.startswith("conv."))
        print("train32 shape, %s: max|dlogp| %.2e, loss rel %.1e, grad err / scale: %.1e outside the CNN (%s), %.1e conv.*"
              % (mode, dl, dloss, worst_rest, [k for e, k in errs if not k.startswith("conv.")][0], worst_conv))
        record_margin("train32_%s_logp" % mode, dl, tol_logp)
        record_margin("train32_%s_loss_rel" % mode, dloss, tol_loss)
        record_margin("train32_%s_grad_rel_scale" % mode, worst_rest, tol_grad)
        record_margin("train32_%s_grad_rel_scale_conv" % mode, worst_conv, 3e-3)
        assert dl <= tol_logp and dloss <= tol_loss, (mode, dl, dloss)
        for e, k in errs:
            assert e <= (3e-3 if k.startswith("conv.") else tol_grad), (mode, k, e)
        del model, out, l2
        torch.cuda.empty_cache()


def test_checkpoint_round_trip_resumes_identically(tmp_path):
    """CTC_Model.save_package (AA/models/model_ctc.py:251-271) -> torch.save -> torch.load -> a FRESH CTC_Model built from the
    package's own fields + load_state_dict, as AA/infer.py:227-254 does -> Adam.load_state_dict(package['optim_dict']), as the
    schedule does with its snapshots (AA/steps/train_ctc.py:236-265): two optimizer steps, checkpoint, and the third step of
    the restored pair is bit-identical to the third step of the uninterrupted run (parameters, BatchNorm buffers, Adam moments);
    the restored model in eval mode gives the posteriors of the original, through the infer path."""
    import torch.nn as nn   # noqa: F401  (the package pickles nn.LSTM / nn.ReLU by reference, as the reference's checkpoints do)
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    from ctc_attention_mispronunciation_amd.train import CTCLoss, Adam
    geom = synth.Geometry(**synth.REFERENCE_256)
    B, T, L = 6, 48, 7
    sd, x, x1, _, tg, il, tl = synth.train_case(geom, 41, B, T, L, 5)
    xd, x1d = _cuda(x), _cuda(x1)
    tgd, ild, tld = torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)
    crit = CTCLoss(reduction="sum")

    def step(model, opt, seed):
        torch.manual_seed(seed)                                  # the dropout draws of this step
        out = model(xd, x1d)
        loss = crit(out, tgd, ild, tld) / B
        opt.zero_grad()
        loss.backward()
        opt.step()
        return float(loss.detach())
    model = _train_model(geom, sd)
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
    losses = [step(model, opt, 100), step(model, opt, 101)]
    path = str(tmp_path / "ctc_best_model.pkl")
    torch.save(CTC_Model.save_package(model, optimizer=opt, epoch={"epoch": 2}, loss_results=losses, dev_loss_results=[1.0, 0.9],
                                      dev_cer_results=[0.1, 0.2]), path)
    l3 = step(model, opt, 102)
    package = torch.load(path, map_location="cpu", weights_only=False)   # a file this test wrote itself
    assert set(package) == {"rnn_param", "add_cnn", "cnn_param", "num_class", "_drop_out", "state_dict", "optim_dict", "epoch",
                            "loss_results", "dev_loss_results", "dev_cer_results"}
    assert set(package["state_dict"]) == set(sd) and package["loss_results"] == losses
    m2 = CTC_Model(rnn_param=package["rnn_param"], add_cnn=package["add_cnn"], cnn_param=package["cnn_param"],
                   num_class=package["num_class"], drop_out=package["_drop_out"])
    m2.load_state_dict(package["state_dict"])
    m2 = m2.cuda().train()
    opt2 = Adam(m2.parameters(), lr=1e-3, weight_decay=5e-4)
    opt2.load_state_dict(package["optim_dict"])
    l3b = step(m2, opt2, 102)
    assert l3b == l3, (l3, l3b)
    for (k, a), (_, b_) in zip(model.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b_), k
    sa, sb = opt.state_dict(), opt2.state_dict()
    assert sa["param_groups"] == sb["param_groups"]
    for i in sa["state"]:
        for name in sa["state"][i]:
            va, vb = sa["state"][i][name], sb["state"][i][name]
            assert torch.equal(torch.as_tensor(va).cpu(), torch.as_tensor(vb).cpu()), (i, name)
    model.eval(); m2.eval()
    with torch.no_grad():
        assert torch.equal(model(xd, x1d), m2(xd, x1d))


def test_run_epoch_over_augmented_dataset_batches(tmp_path, capsys):
    """SURVEY 8(f) #4 on the GPU box: the reference's training loop body (AA/steps/train_ctc.py:28-105) over
    SpeechDataLoader(SpeechDataset(train=True)) batches -- features read back from a Kaldi ark the package wrote, spec_augment on the raw
    frames and data_enhancement on the canonical ids per item (AA/utils/data_loader.py:132-137, AA/utils/tools.py:229-255,290-359), the
    reference's collate -- through the HIP train-mode forward, CTC loss, backward and Adam; then a validation pass over the
    un-augmented split.  The loop prints the reference's progress lines; the loss falls over the epochs."""
    import random
    import types
    from ctc_attention_mispronunciation_amd.utils import data_loader as dl, fbank as fb
    from ctc_attention_mispronunciation_amd.steps.train_ctc import run_epoch, build_training
    geom = synth.Geometry(**synth.REFERENCE_256)
    rs = np.random.Generator(np.random.PCG64(12))
    phones = [synth.phone_table_41()[i] for i in range(2, 43)]
    (tmp_path / "units").write_text("\n".join("%s %s" % (p, p) for p in phones) + "\n")
    feats, lab, trn = {}, [], []
    for i in range(12):
        n = int(rs.integers(60, 101))
        feats["u%02d" % i] = rs.standard_normal((n, 81)).astype(np.float32)
        k = int(rs.integers(3, 7))
        ph = [phones[int(j)] for j in rs.integers(1, 40, size=k)]
        lab.append("u%02d %s" % (i, " ".join(ph)))
        trn.append("u%02d %s" % (i, " ".join(ph)))
    fb.write_ark_scp(str(tmp_path / "f.ark"), str(tmp_path / "f.scp"), feats)
    (tmp_path / "lab").write_text("\n".join(lab) + "\n")
    (tmp_path / "trn").write_text("\n".join(trn) + "\n")
    vocab = dl.Vocab(str(tmp_path / "units"))
    assert vocab.n_words == 43
    opts = types.SimpleNamespace(left_ctx=0, right_ctx=2, n_skip_frame=2, n_downsample=2, feature_type="fbank", mel=False)
    mk = lambda train: dl.SpeechDataset(vocab, str(tmp_path / "f.scp"), str(tmp_path / "lab"), str(tmp_path / "trn"), opts, train=train)   # noqa: E731
    random.seed(5); np.random.seed(5); torch.manual_seed(5)
    train_loader = dl.SpeechDataLoader(mk(True), batch_size=4, shuffle=True)
    dev_loader = dl.SpeechDataLoader(mk(False), batch_size=4, shuffle=False)
    sd = synth.synth_state_dict(synth.Geometry(**dict(synth.REFERENCE_256, num_class=43)), seed=3)
    model = _train_model(synth.Geometry(**dict(synth.REFERENCE_256, num_class=43)), sd)
    loss_fn, opt = build_training(model)
    dev = torch.device("cuda")
    hist = []
    for ep in range(4):
        acc, loss = run_epoch(ep, model, train_loader, loss_fn, dev, optimizer=opt, print_every=2, is_training=True)
        hist.append(loss)
    vacc, vloss = run_epoch(4, model, dev_loader, loss_fn, dev, optimizer=None, is_training=False)
    text = capsys.readouterr().out
    assert "Epoch = 0, step = 2, total_loss" in text and "Epoch 3 Train done" in text and "Epoch 4 Valid done" in text
    assert np.isfinite(hist).all() and hist[-1] < hist[0], hist
    assert np.isfinite(vloss) and 0.0 <= vacc <= 1.0 or vacc < 0     # (1 - error rate can be negative: more errors than tokens)


def test_ctc_loss_module_matches_nn_ctcloss():
    """The nn.CTCLoss-shaped callable (train_ctc.py:72,186): value and autograd gradient against the G5 goldens (torch's
    CTCLoss(sum) + backward), then 'mean' / 'none', 1-D concatenated targets and zero_infinity against torch on the CPU."""
    from ctc_attention_mispronunciation_amd.train import CTCLoss
    g = npz("g5_ctc.npz")
    for meta in jload("g5_ctc.json"):
        i = meta["i"]
        if not np.isfinite(g["nll%d" % i]).all():
            continue
        lp = _cuda(g["logp%d" % i]).requires_grad_(True)
        loss = CTCLoss(reduction="sum")(lp, torch.from_numpy(g["tg%d" % i]), torch.from_numpy(g["il%d" % i]), torch.from_numpy(g["tl%d" % i]))
        assert abs(float(loss) - meta["loss"]) <= 2e-6 * abs(meta["loss"]) + 1e-4
        loss.backward()
        np.testing.assert_allclose(lp.grad.cpu().numpy(), g["grad%d" % i], rtol=0, atol=TOL)
    i = 7                                                    # the case with an infeasible row
    lp_np, tg, il, tl = g["logp%d" % i], g["tg%d" % i], g["il%d" % i], g["tl%d" % i]
    for red in ("mean", "none", "sum"):
        for zi in (False, True):
            ref = torch.nn.CTCLoss(reduction=red, zero_infinity=zi)(torch.from_numpy(lp_np), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl))
            got = CTCLoss(reduction=red, zero_infinity=zi)(_cuda(lp_np), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)).cpu()
            np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=2e-6, atol=1e-4)
    flat = torch.cat([torch.from_numpy(tg[b, :tl[b]]) for b in range(len(tl))])
    a = CTCLoss(reduction="none")(_cuda(lp_np), flat, il.tolist(), tl.tolist()).cpu().numpy()
    b = CTCLoss(reduction="none")(_cuda(lp_np), torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)).cpu().numpy()
    np.testing.assert_array_equal(a, b)


def test_adam_matches_torch_optim_adam():
    """mdd_adam_step behind a torch.optim-compatible class against torch.optim.Adam (CPU) over several steps with the
    reference's settings (lr 1e-3, weight_decay 5e-4; train_ctc.py:187), state_dict round trip included."""
    from ctc_attention_mispronunciation_amd.train import Adam
    rs = np.random.Generator(np.random.PCG64(1))
    shapes = [(7,), (33, 5), (128, 129), (3, 4, 5, 6)]
    p_ref = [torch.nn.Parameter(torch.from_numpy(rs.standard_normal(s).astype(np.float32))) for s in shapes]
    p_hip = [torch.nn.Parameter(p.detach().clone().cuda()) for p in p_ref]
    o_ref = torch.optim.Adam(p_ref, lr=1e-3, weight_decay=5e-4)
    o_hip = Adam(p_hip, lr=1e-3, weight_decay=5e-4)
    for step in range(6):
        for a, b in zip(p_ref, p_hip):
            gnp = (rs.standard_normal(a.shape) * (10.0 if step == 2 else 1.0)).astype(np.float32)
            a.grad = torch.from_numpy(gnp); b.grad = torch.from_numpy(gnp).cuda()
        o_ref.step(); o_hip.step()
        if step == 3:                                        # halve the rate as the schedule does (train_ctc.py:215-268) and reload the state
            for grp in o_ref.param_groups + o_hip.param_groups:
                grp["lr"] *= 0.5
            o_hip.load_state_dict(o_hip.state_dict())
        for a, b in zip(p_ref, p_hip):
            np.testing.assert_allclose(b.detach().cpu().numpy(), a.detach().numpy(), rtol=2e-6, atol=2e-7)
    sd_ref, sd_hip = o_ref.state_dict(), o_hip.state_dict()
    assert set(sd_ref["state"][0].keys()) <= set(sd_hip["state"][0].keys())


def test_train_mode_generated_masks_and_full_loop():
    """Without given masks the library draws them (counter-based generator): same seed -> same bits, keep-rate 1 - p; and a
    short training loop of the drop-in pieces (model.train() forward, CTCLoss, backward, Adam) lowers the loss."""
    from ctc_attention_mispronunciation_amd.train import CTCLoss, Adam
    geom = synth.Geometry(**synth.REFERENCE_256)
    sd, x, x1, _, tg, il, tl = synth.train_case(geom, 5, 4, 32, 6, 4)
    model = _train_model(geom, sd)
    xd, x1d = _cuda(x), _cuda(x1)
    torch.manual_seed(3)
    a = model(xd, x1d).detach().clone()
    torch.manual_seed(3)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})     # undo the running-statistics update
    b = model(xd, x1d).detach().clone()
    assert torch.equal(a, b)
    c = model(xd, x1d).detach()
    assert not torch.equal(a, c)                              # the next draw differs
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
    crit = CTCLoss(reduction="sum")
    losses = []
    for _ in range(8):
        out = model(xd, x1d)
        loss = crit(out, torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)) / 4
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0], losses
    model.eval()
    with torch.no_grad():
        ev = model(xd, x1d)                                   # the eval path picks up the trained weights (its packed copies were stale)
    assert torch.isfinite(ev).all() and float(torch.exp(ev.double()).sum(-1).sub(1).abs().max()) < 1e-5


def test_train_variant_soak_and_eval_consistency():
    """60 optimizer steps in the flagged split-bf16 variant (both persistent recurrences, 2 x 5 launches per step, device gate taken and
    released each time): no hand-off time-out (mdd_train_sync raises on one), the loss falls, and the eval path afterwards (which
    re-packs the trained weights) gives normalised posteriors."""
    from ctc_attention_mispronunciation_amd.train import CTCLoss, Adam
    geom = synth.Geometry(**synth.REFERENCE)
    B, T, L = 24, 64, 8
    sd, x, x1, _, tg, il, tl = synth.train_case(geom, 11, B, T, L, 5)
    model = _train_model(geom, sd)
    model.train_precision = "bf16x3"
    xd, x1d = _cuda(x), _cuda(x1)
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
    crit = CTCLoss(reduction="sum")
    tgd, ild, tld = torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)
    losses = []
    for _ in range(60):
        out = model(xd, x1d)
        loss = crit(out, tgd, ild, tld) / B
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[-1] < 0.7 * losses[0], (losses[0], losses[-1])
    model.eval()
    with torch.no_grad():
        ev = model(xd, x1d)
    assert torch.isfinite(ev).all() and float(torch.exp(ev.double()).sum(-1).sub(1).abs().max()) < 1e-5


def test_train_variant_tracks_exact_mode_over_steps():
    """The same 25 optimizer steps (same initial weights, batch, seeded dropout draws) in exact fp32 and in the flagged split-bf16 variant:
    the two loss curves stay within 1 % of the initial loss of each other over the first ten steps (5 % to the end, where the batch is being
    memorised and the trajectories are sensitive to any rounding) and both fall below a tenth of it."""
    from ctc_attention_mispronunciation_amd.train import CTCLoss, Adam
    geom = synth.Geometry(**synth.REFERENCE)
    B, T, L = 16, 64, 8
    sd, x, x1, _, tg, il, tl = synth.train_case(geom, 21, B, T, L, 5)
    xd, x1d = _cuda(x), _cuda(x1)
    tgd, ild, tld = torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl)
    curves = {}
    for mode in ("f32", "bf16x3"):
        model = _train_model(geom, sd)
        model.train_precision = mode
        opt = Adam(model.parameters(), lr=1e-3, weight_decay=5e-4)
        crit = CTCLoss(reduction="sum")
        torch.manual_seed(1234)
        cur = []
        for _ in range(25):
            out = model(xd, x1d)
            loss = crit(out, tgd, ild, tld) / B
            opt.zero_grad()
            loss.backward()
            opt.step()
            cur.append(float(loss.detach()))
        curves[mode] = np.asarray(cur)
    print("f32   ", np.round(curves["f32"], 3))
    print("bf16x3", np.round(curves["bf16x3"], 3))
    rel = np.abs(curves["bf16x3"] - curves["f32"]) / curves["f32"][0]      # against the initial loss: the end of the curves is a memorised batch
    assert rel[:10].max() < 1e-2 and rel.max() < 5e-2
    assert curves["f32"][-1] < 0.1 * curves["f32"][0] and curves["bf16x3"][-1] < 0.1 * curves["bf16x3"][0]


def test_run_epoch_mirror_trains_and_validates():
    """steps/train_ctc.run_epoch (the reference's loop, train_ctc.py:28-105) over an in-memory loader of create_input batches:
    a training epoch then a validation epoch; returns (accuracy, mean loss), parameters move only in training."""
    from ctc_attention_mispronunciation_amd.steps.train_ctc import run_epoch, build_training
    from ctc_attention_mispronunciation_amd.utils.data_loader import create_input
    geom = synth.Geometry(**synth.REFERENCE_256)
    sd = synth.synth_state_dict(geom, seed=9)
    model = _train_model(geom, sd)
    rs = np.random.Generator(np.random.PCG64(4))
    batches = []
    for k in range(3):
        items = []
        for u in range(4):
            T = int(rs.integers(10, 17)) * 2
            items.append((torch.from_numpy(rs.standard_normal((T, 243)).astype(np.float32)), torch.from_numpy(rs.integers(2, 44, size=int(rs.integers(2, 5)))),
                          torch.from_numpy(rs.integers(2, 44, size=int(rs.integers(3, 8)))), "u%d_%d" % (k, u)))
        batches.append(create_input(items))
    loss_fn, opt = build_training(model)
    w0 = model.fc[1].weight.detach().clone()
    acc, loss = run_epoch(1, model, batches, loss_fn, "cuda", optimizer=opt, print_every=2, is_training=True)
    assert np.isfinite(loss) and acc <= 1.0 and not torch.equal(w0, model.fc[1].weight)
    w1 = model.fc[1].weight.detach().clone()
    acc2, loss2 = run_epoch(1, model, batches, loss_fn, "cuda", optimizer=None, is_training=False)
    assert np.isfinite(loss2) and torch.equal(w1, model.fc[1].weight) and not model.training


def _ragged_batches(geom, shapes, seed):
    """Reference-style batches of different padded lengths: [(x [b,T_g,F], x1 [b,L_g], frac)], every utterance zero-padded
    inside its batch as the collate does (synth_batch ragged=True)."""
    out = []
    for k, (b, T, L) in enumerate(shapes):
        x, x1, frac, _ = synth.synth_batch(geom, B=b, T=T, L=L, seed=seed + 31 * k, ragged=True)
        out.append((x, x1, frac))
    return out


@pytest.mark.parametrize("precision,lstm", [("bf16x3", None), ("bf16x3", "x3"), ("f32", None), ("f32x6", None)])
@pytest.mark.parametrize("H", [384, 256])
def test_fused_batches_of_different_lengths_equal_their_own_runs(precision, lstm, H, monkeypatch):
    """mdd_forward_fused: batches padded to DIFFERENT lengths T_g / L_g ride one launch sequence; every utterance's posteriors
    must equal, bit for bit, what mdd_forward gives for its batch alone (the reference masks nothing, so its batch's padded
    lengths are part of an utterance's result: reverse-direction start, attention over l < L_g).  Persistent BiLSTM, the
    per-step split-bf16 kernels and the exact-fp32 mode."""
    if lstm:
        monkeypatch.setenv("MDD_LSTM", lstm)
    geom = synth.Geometry(**dict(synth.REFERENCE, hidden=H))
    sd = synth.synth_state_dict(geom, seed=1234)
    shapes = [(5, 120, 9), (3, 64, 4), (7, 100, 12), (2, 120, 12), (4, 30, 1)]
    batches = _ragged_batches(geom, shapes, seed=7)
    m = _hip().HipModel(geom, sd, precision=precision)
    alone = [m.forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy() for x, x1, _ in batches]
    Bt, Tm, Lm = sum(s[0] for s in shapes), max(s[1] for s in shapes), max(s[2] for s in shapes)
    X = np.zeros((Bt, Tm, geom.feat), dtype=np.float32)
    X1 = np.zeros((Bt, Lm), dtype=np.int64)
    frames, canon = np.zeros(Bt, dtype=np.int32), np.zeros(Bt, dtype=np.int32)
    r = 0
    for (x, x1, _), (b, T, L) in zip(batches, shapes):
        X[r:r + b, :T] = x; X1[r:r + b, :L] = x1; frames[r:r + b] = T // 2; canon[r:r + b] = L
        r += b
    fused = m.forward_fused(_cuda(X), _cuda(X1), _cuda(frames), _cuda(canon), sync_errors=True).cpu().numpy()
    r = 0
    for lp, (b, T, L) in zip(alone, shapes):
        np.testing.assert_array_equal(fused[:T // 2, r:r + b], lp)
        r += b
    # run to run (replays of the graph the first call captured): every DEFINED row (t < frames[b]; rows beyond are undefined by the interface and
    # may depend on what the workspace held).  This is the check that caught graph memset nodes not preceding the persistent layer kernels
    # (profiles/round3_lstm_ordering.txt): the single-batch forwards above leave the exchange buffer non-zero, a replay then started on it.
    for _ in range(3):
        again = m.forward_fused(_cuda(X), _cuda(X1), _cuda(frames), _cuda(canon), sync_errors=True).cpu().numpy()
        for b in range(Bt):
            np.testing.assert_array_equal(again[:frames[b], b], fused[:frames[b], b])


def test_fused_batches_full_size_and_reference_golden():
    """Bench-sized fusion (8 ragged 64-utterance batches, 10 s, the multi-tile persistent BiLSTM): three of the batches checked
    against their own runs bit for bit; and the G9 reference golden batch (T'=250) riding along with a shorter one still
    decodes to the reference's strings."""
    from tests.helpers import chain_inputs
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=1234)
    rs = np.random.Generator(np.random.PCG64(5))
    shapes = [(64, int(rs.integers(440, 501)) // 2 * 2, int(rs.integers(20, 41))) for _ in range(8)]
    batches = _ragged_batches(geom, shapes, seed=99)
    m = _hip().HipModel(geom, sd, precision="bf16x3")
    Bt, Tm, Lm = 512, max(s[1] for s in shapes), max(s[2] for s in shapes)
    X = torch.zeros((Bt, Tm, geom.feat), device="cuda")
    X1 = torch.zeros((Bt, Lm), dtype=torch.int64, device="cuda")
    frames, canon = torch.zeros(Bt, dtype=torch.int32, device="cuda"), torch.zeros(Bt, dtype=torch.int32, device="cuda")
    for g_, ((x, x1, _), (b, T, L)) in enumerate(zip(batches, shapes)):
        X[64 * g_:64 * g_ + 64, :T] = _cuda(x); X1[64 * g_:64 * g_ + 64, :L] = _cuda(x1)
        frames[64 * g_:64 * g_ + 64] = T // 2; canon[64 * g_:64 * g_ + 64] = L
    fused = m.forward_fused(X, X1, frames, canon, sync_errors=True)
    for g_ in (0, 3, 7):
        x, x1, _ = batches[g_]
        own = m.forward(_cuda(x), _cuda(x1), sync_errors=True)
        assert torch.equal(fused[:shapes[g_][1] // 2, 64 * g_:64 * g_ + 64], own), g_
    # the reference's own T'=250 batch (G9) fused with a short one
    meta = jload("g9_chain.json")[0]
    ref = npz("g9_chain.npz")[meta["tag"] + "_logp"]
    geom9, sd9, x, x1, frac, _ = chain_inputs(meta)
    m9 = _hip().HipModel(geom9, sd9, precision="bf16x3")
    xs, x1s, _ = _ragged_batches(geom9, [(2, 64, 5)], seed=3)[0]
    B9 = x.shape[0]
    X = np.zeros((B9 + 2, 500, geom9.feat), dtype=np.float32); X1 = np.zeros((B9 + 2, 40), dtype=np.int64)
    X[:B9] = x; X1[:B9] = x1; X[B9:, :64] = xs; X1[B9:, :5] = x1s
    fr = np.array([250] * B9 + [32, 32], dtype=np.int32); cn = np.array([40] * B9 + [5, 5], dtype=np.int32)
    lp = m9.forward_fused(_cuda(X), _cuda(X1), _cuda(fr), _cuda(cn), sync_errors=True).cpu().numpy()
    np.testing.assert_allclose(lp[:, :B9], ref, rtol=0, atol=TOL)
    np.testing.assert_array_equal(lp[:32, B9:], m9.forward(_cuda(xs), _cuda(x1s)).cpu().numpy())


def test_fused_batches_edge_shapes():
    """mdd_forward_fused at the edges: single-utterance batches, the shortest legal batch (one posterior frame, one canonical
    phoneme), a batch that alone fills the common shape, 17 + 1 + 33 rows (team tiles that are not multiples of 16)."""
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=31)
    shapes = [(17, 20, 3), (1, 2, 1), (33, 8, 5), (1, 20, 5)]
    batches = _ragged_batches(geom, shapes, seed=77)
    for precision in ("bf16x3", "f32"):
        m = _hip().HipModel(geom, sd, precision=precision)
        Bt, Tm, Lm = sum(s[0] for s in shapes), max(s[1] for s in shapes), max(s[2] for s in shapes)
        X = np.zeros((Bt, Tm, geom.feat), dtype=np.float32); X1 = np.zeros((Bt, Lm), dtype=np.int64)
        fr, cn = np.zeros(Bt, dtype=np.int32), np.zeros(Bt, dtype=np.int32)
        r = 0
        for (x, x1, _), (b, T, L) in zip(batches, shapes):
            X[r:r + b, :T] = x; X1[r:r + b, :L] = x1; fr[r:r + b] = T // 2; cn[r:r + b] = L
            r += b
        fused = m.forward_fused(_cuda(X), _cuda(X1), _cuda(fr), _cuda(cn), sync_errors=True).cpu().numpy()
        r = 0
        for (x, x1, _), (b, T, L) in zip(batches, shapes):
            own = m.forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy()
            np.testing.assert_array_equal(fused[:T // 2, r:r + b], own)
            np.testing.assert_allclose(own, oracle.forward(sd, x, x1), rtol=0, atol=TOL)
            r += b
