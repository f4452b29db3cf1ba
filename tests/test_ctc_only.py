"""The CTC-only model (the reference's egs/cnn-rnn-ctc baseline) on the GPU decode path: a handle of mdd_create_ctc behind HipModel,
models.cnn_rnn.CTC_Model and infer.  CPU side: tests/test_ctc_only_reference.py; helpers and cases: tests/ctc_only_cases.py.

Bounds: every log-prob comparison is <= 1e-4 (README's parity tolerance, ctc_only_cases.TOL) in every arithmetic mode, against the reference's
own fp32 output (G15) and against the float64 restatement; what is measured is recorded (tests/helpers.record_margin; tools/ctc_only_margins.py
writes profiles/ctc_only_margins.json).  Everything said to be the same bits is compared with assert_array_equal."""
import ctypes as C
import io
import os
import shutil

import numpy as np
import pytest
import torch

from tests import ctc_only_cases as cc
from tests.helpers import GOLD, jload, npz, record_margin

pytestmark = pytest.mark.gpu
PRECISIONS = ("f32x6", "f32", "bf16x3")
TEXT_STAGES = ("embed", "gemm_text", "lstm_text", "gemm_key", "gemm_score", "attn_tail")


def _synth():
    from ctc_attention_mispronunciation_amd import synth
    return synth


def _hip():
    from ctc_attention_mispronunciation_amd import hip_model
    return hip_model


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _model(geom, sd, precision, taps=False):
    m = _hip().HipModel(geom, sd, precision=precision, taps=taps)
    assert _lib().lib().mdd_is_ctc_only(m.handle) == (1 if geom.ctc_only else 0)
    return m


def _lib():
    from ctc_attention_mispronunciation_amd import _lib as lib
    return lib


# ----------------------------------------------------------------------------- golden parity
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("tag", ["tiny", "h256", "h384"])
def test_golden_parity(tag, precision):
    """HipModel on G15's inputs against the reference CTC_Model's own fp32 log-probs, <= 1e-4 in every mode; at H = 384 the greedy and
    beam-10 decode of the library's own log-probs are the reference decoders' strings.  Measured: <= 3.4e-6 in modes f32 and f32x6, <= 6.7e-6 in bf16x3."""
    synth = _synth()
    meta, g = jload("g15_ctc_only.json"), npz("g15_ctc_only.npz")
    case = [c for c in meta["cases"] if c["tag"] == tag][0]
    geom = synth.Geometry(ctc_only=True, **case["geom"])
    m = _model(geom, synth.synth_state_dict(geom, seed=case["seed"]), precision)
    assert m.precision == cc.expected_precision(geom, precision)
    logp = m.forward(_cuda(g[tag + "_x"]), None, sync_errors=True)
    err = float(np.abs(logp.cpu().numpy() - g[tag + "_logp"]).max())
    record_margin("g15_%s_%s_logp" % (tag, precision), err, cc.TOL)
    print("G15 %s %s: max|logp - reference| = %.3e" % (tag, precision, err))
    assert err <= cc.TOL, (tag, precision, err)
    if tag == "h384":
        from ctc_attention_mispronunciation_amd.utils.ctcDecoder import GreedyDecoder, BeamDecoder
        i2c = synth.phone_table_41()
        assert GreedyDecoder(i2c, space_idx=-1, blank_index=0).decode(logp, case["lens"]) == case["greedy"]
        beam = BeamDecoder(i2c, beam_width=10, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=0.0)
        assert beam.decode(logp, case["lens"]) == case["beam10"]
    m.close()


# ----------------------------------------------------------------------------- against float64 at the tail's edges
def measure_case(name, kwargs, shapes=cc.SHAPES, seed=31):
    """{"B<B>_T<T>_<mode>": (max|logp - float64|, max|logp - float64 tail of the tapped last layer|)} for one geometry: the float64
    forward once per shape, one handle per mode.  Asserts what is not a figure: the mode in effect, finite outputs, rows that sum to 1."""
    synth = _synth()
    geom = cc.geometry(kwargs)
    sd = synth.synth_state_dict(geom, seed=seed)
    xs = [cc.draw_batch(geom, B, T, seed=seed + B) for B, T in shapes]
    refs = [cc.forward_f64(sd, x) for x in xs]
    out = {}
    for precision in PRECISIONS:
        m = _model(geom, sd, precision)
        assert m.precision == cc.expected_precision(geom, precision), (name, precision, m.precision)   # a fallback is reported (plan.h)
        for (B, T), x, ref in zip(shapes, xs, refs):
            logp = m.forward(_cuda(x), None, sync_errors=True).cpu().numpy()
            assert logp.shape == ref.shape == (T // 2, B, geom.num_class) and np.isfinite(logp).all()
            assert float(np.abs(np.exp(logp.astype(np.float64)).sum(-1) - 1).max()) < 1e-5
            last = m.tap("rnn%d" % (geom.layers - 1)).view(T // 2, B, 2 * geom.hidden).cpu().numpy()
            tail = cc.tail_f64(sd, last)
            out["B%d_T%d_%s" % (B, T, precision)] = (float(np.abs(logp - ref).max()), float(np.abs(logp - tail).max()))
        m.close()
    return out


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_against_float64_at_the_tail_edges(name):
    """Every geometry of ctc_only_cases.CASES (both forms of ctc_tail: 2H = 768, 512, 256, 128 on the matrix cores with C = 45, 48, 2; C = 49,
    101, 12, 7 and 2H = 40, 16 scalar) at R = 21, 561 and 1 rows, every mode: <= 1e-4 from the float64 forward.  And the tail alone: BN +
    Linear + log-softmax evaluated in float64 on the host from the tapped fp32 output of the last layer, <= 1e-4 from the log-probs --
    ctc_tail's own error, apart from the recurrences'.  Measured over all cases (profiles/ctc_only_margins.json): forward <= 1.5e-6 in modes f32 and
    f32x6, <= 1.4e-5 in bf16x3; the tail alone <= 1.5e-6 in every mode."""
    kwargs, form = cc.CASES[name]
    assert cc.tail_form(cc.geometry(kwargs)) == form
    for key, (err, tail_err) in sorted(measure_case(name, kwargs).items()):
        record_margin("ctc_only_%s_%s" % (name, key), err, cc.TOL)
        record_margin("ctc_only_tail_%s_%s" % (name, key), tail_err, cc.TOL)
        print("%s %s: forward %.3e, tail alone %.3e" % (name, key, err, tail_err))
        assert err <= cc.TOL, (name, key, err)
        assert tail_err <= cc.TOL, (name, key, tail_err)


@pytest.mark.parametrize("name", sorted(cc.LAYER_CASES))
def test_one_and_six_layers_against_float64(name):
    """layers = 1 (the only layer hands its raw output to the tail) and layers = 6, at R = 561."""
    for key, (err, tail_err) in sorted(measure_case(name, cc.LAYER_CASES[name][0], shapes=cc.SHAPES[1:2]).items()):
        record_margin("ctc_only_%s_%s" % (name, key), err, cc.TOL)
        print("%s %s: forward %.3e, tail alone %.3e" % (name, key, err, tail_err))
        assert err <= cc.TOL and tail_err <= cc.TOL, (name, key, err, tail_err)


# ----------------------------------------------------------------------------- nothing else moved
@pytest.mark.parametrize("name,B,T", [("H384", 3, 14), ("H384", 17, 66), ("tiny", 3, 14)])
def test_acoustic_stages_are_the_attention_handles_bits(name, B, T):
    """The same conv / BiLSTM weights in a CTC-only handle and in an attention handle: the taps conv1 and every rnn<i> are bit-identical
    in each mode -- the acoustic stages are the attention forward's, unchanged."""
    synth = _synth()
    geom = cc.geometry(cc.CASES[name][0])
    sd = synth.synth_state_dict(geom, seed=41)
    ageom, asd = cc.attention_twin(geom, sd, seed=42)
    x = _cuda(cc.draw_batch(geom, B, T, seed=43))
    x1 = torch.ones((B, 5), dtype=torch.int64, device="cuda")
    for precision in PRECISIONS:
        mc, ma = _model(geom, sd, precision, taps=True), _model(ageom, asd, precision, taps=True)
        assert mc.precision == ma.precision
        mc.forward(x, None, sync_errors=True)
        ma.forward(x, x1, sync_errors=True)
        for tap in ["conv1"] + ["rnn%d" % i for i in range(geom.layers)]:
            np.testing.assert_array_equal(mc.tap(tap).cpu().numpy(), ma.tap(tap).cpu().numpy(), err_msg="%s %s" % (precision, tap))
        mc.close(); ma.close()


# ----------------------------------------------------------------------------- forward variants
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_variants_give_the_same_bits(precision):
    """forward_raw = mdd_stack_skip + forward; forward_fused with two groups (T = 32 and T = 20) gives every row t < frames[b] the bits of
    its own group's forward; replays of the captured graph repeat themselves."""
    from ctc_attention_mispronunciation_amd.utils.data_loader import stack_features
    synth = _synth()
    geom = cc.geometry({})
    m = _model(geom, synth.synth_state_dict(geom, seed=51), precision)
    raw = _cuda(synth.synth_raw_features(3, T_raw=61, seed=52))
    np.testing.assert_array_equal(m.forward_raw(raw, None, sync_errors=True).cpu().numpy(),
                                  m.forward(stack_features(raw), None, sync_errors=True).cpu().numpy())
    groups = [cc.draw_batch(geom, 3, 32, seed=53), cc.draw_batch(geom, 2, 20, seed=54)]
    alone = [m.forward(_cuda(x), None, sync_errors=True).cpu().numpy() for x in groups]
    X = np.zeros((5, 32, geom.feat), dtype=np.float32)
    X[:3], X[3:, :20] = groups[0], groups[1]
    frames = _cuda(np.array([16, 16, 16, 10, 10], dtype=np.int32))
    fused = m.forward_fused(_cuda(X), None, frames, None, sync_errors=True).cpu().numpy()
    np.testing.assert_array_equal(fused[:, :3], alone[0])
    np.testing.assert_array_equal(fused[:10, 3:], alone[1])
    for _ in range(2):       # replays of the graph the first call captured
        again = m.forward_fused(_cuda(X), None, frames, None, sync_errors=True).cpu().numpy()
        np.testing.assert_array_equal(again[:, :3], fused[:, :3])
        np.testing.assert_array_equal(again[:10, 3:], fused[:10, 3:])
    xg = _cuda(groups[0])
    np.testing.assert_array_equal(m.forward(xg, None, sync_errors=True).cpu().numpy(), alone[0])
    np.testing.assert_array_equal(m.forward(xg, None, sync_errors=True).cpu().numpy(), alone[0])
    m.close()


# ----------------------------------------------------------------------------- ignored inputs
def test_canonical_inputs_are_ignored():
    """x1 = NULL and an x1 full of ids no table has (10^6) give the same bits, at any L, and mdd_sync reports nothing; the text-side taps
    do not exist; the profile lists the acoustic stages and ctc_tail, none of the six text / attention stages."""
    synth = _synth()
    geom = cc.geometry({})
    m = _model(geom, synth.synth_state_dict(geom, seed=61), None, taps=True)
    x = _cuda(cc.draw_batch(geom, 3, 14, seed=62))
    a = m.forward(x, None, sync_errors=True).cpu().numpy()
    for L in (4, 5000):      # (past every canonical-length limit of the attention handle)
        bad = torch.full((3, L), 10 ** 6, dtype=torch.int64, device="cuda")
        np.testing.assert_array_equal(m.forward(x, bad, sync_errors=True).cpu().numpy(), a)
        assert _lib().lib().mdd_sync(m.handle, _lib().current_stream_ptr()) == 0
    for tap in ("text", "key", "score"):
        assert not _lib().lib().mdd_tap(m.handle, tap.encode(), None)
        with pytest.raises(KeyError):
            m.tap(tap)
    assert m.tap("conv1").numel() == 7 * 3 * geom.rnn_in and m.tap("rnn0").numel() == 7 * 3 * 2 * geom.hidden
    prof = m.profile(x, None)
    names = [p[0] for p in prof]
    assert _lib().lib().mdd_forward_num_stages(m.handle) == len(names) == 2 + 2 * geom.layers + 1
    assert names[-1] == "ctc_tail" and prof[-1][2] == 1 and prof[-1][1] > 0
    assert not set(names) & set(TEXT_STAGES)
    assert names[2:-1] == [s % n for n in range(geom.layers) for s in ("gemm_ih%d", "lstm%d")]
    ageom, asd = cc.attention_twin(geom, synth.synth_state_dict(geom, seed=61), seed=63)
    ma = _model(ageom, asd, None)
    anames = [p[0] for p in ma.profile(x, torch.ones((3, 4), dtype=torch.int64, device="cuda"))]
    assert anames[:len(names) - 1] == names[:-1] and anames[len(names) - 1:] == list(TEXT_STAGES)     # the acoustic stages, unchanged
    m.close(); ma.close()


# ----------------------------------------------------------------------------- errors
def _load(lib, h, key, arr):
    a = np.ascontiguousarray(arr, dtype=np.float32)
    shape = (C.c_int64 * max(1, a.ndim))(*a.shape)
    return lib.mdd_load_weight(h, key.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim)


def test_refusals_name_their_reason_and_leave_a_usable_library():
    """mdd_create_ctc with an embedding, an attention key, a 4H-wide classifier, a finalize with fc.0.bias missing: each refused with the
    documented status and the name in mdd_last_error(); after each the handle is destroyed cleanly and a fresh one works."""
    synth = _synth()
    L = _lib()
    lib = L.lib()
    geom = cc.geometry(cc.CASES["tiny"][0])
    sd = synth.synth_state_dict(geom, seed=71)
    x = _cuda(cc.draw_batch(geom, 3, 14, seed=72))
    want = cc.forward_f64(sd, x.cpu().numpy())

    def fresh_works():
        m = _model(geom, sd, None)
        assert float(np.abs(m.forward(x, None, sync_errors=True).cpu().numpy() - want).max()) <= cc.TOL
        m.close()

    def create():
        h = C.c_void_p()
        cfg = L.MddConfig(feat=geom.feat, hidden=geom.hidden, layers=geom.layers, num_class=geom.num_class, channels=geom.channels,
                          emb_rows=0, emb_dim=0, bn_eps=1e-5)
        assert lib.mdd_create_ctc(C.byref(cfg), 0, C.byref(h)) == 0 and h.value and lib.mdd_is_ctc_only(h) == 1
        return h

    cfg = L.MddConfig(feat=geom.feat, hidden=geom.hidden, layers=geom.layers, num_class=geom.num_class, channels=geom.channels,
                      emb_rows=44, emb_dim=0, bn_eps=1e-5)
    h = C.c_void_p()
    assert lib.mdd_create_ctc(C.byref(cfg), 0, C.byref(h)) == -1 and not h.value
    assert "emb_rows" in lib.mdd_last_error().decode()
    cfg.emb_rows, cfg.emb_dim = 0, 12
    assert lib.mdd_create_ctc(C.byref(cfg), 0, C.byref(h)) == -1 and "emb_dim" in lib.mdd_last_error().decode()
    cfg.emb_dim = 0
    assert lib.mdd_create(C.byref(cfg), 0, C.byref(h)) == -1 and "emb_rows" in lib.mdd_last_error().decode()      # mdd_create as before
    fresh_works()

    h = create()
    assert _load(lib, h, "embeds.weight", np.zeros((7, 12))) == -1 and "embeds.weight" in lib.mdd_last_error().decode()
    assert _load(lib, h, "lstm_embeds.weight_ih_l0", np.zeros((32, 12))) == -1 and "lstm_embeds.weight_ih_l0" in lib.mdd_last_error().decode()
    assert _load(lib, h, "score.weight", np.zeros((16, 16))) == -1 and "score.weight" in lib.mdd_last_error().decode()
    lib.mdd_destroy(h)
    fresh_works()

    h = create()
    assert _load(lib, h, "fc.1.weight", np.zeros((geom.num_class, 4 * geom.hidden))) == -1            # the attention model's width
    assert "fc.1.weight" in lib.mdd_last_error().decode()
    assert _load(lib, h, "fc.1.weight", sd["fc.1.weight"]) == 0
    assert _load(lib, h, "fc.0.num_batches_tracked", np.zeros(())) == 0                                 # ignored, as ever
    lib.mdd_destroy(h)
    fresh_works()

    h = create()
    for k, v in sd.items():
        if v.dtype.kind == "f" and k != "fc.0.bias":
            assert _load(lib, h, k, v) == 0, k
    assert lib.mdd_finalize_weights(h) == -3 and "fc.0.bias" in lib.mdd_last_error().decode()          # MDD_ERR_STATE
    out = torch.empty((7, 3, geom.num_class), device="cuda")
    assert lib.mdd_forward(h, C.c_void_p(x.data_ptr()), 3, 14, None, 0, C.c_void_p(out.data_ptr()), None) == -3      # not finalized
    assert _load(lib, h, "fc.0.bias", sd["fc.0.bias"]) == 0 and lib.mdd_finalize_weights(h) == 0       # ... and the same handle recovers
    assert lib.mdd_forward(h, C.c_void_p(x.data_ptr()), 3, 14, None, 0, C.c_void_p(out.data_ptr()), None) == 0
    assert lib.mdd_sync(h, None) == 0
    assert float(np.abs(out.cpu().numpy() - want).max()) <= cc.TOL
    lib.mdd_destroy(h)
    fresh_works()


# ----------------------------------------------------------------------------- drop-in
def _drop_in(geom, sd):
    import torch.nn as nn
    from ctc_attention_mispronunciation_amd.models.cnn_rnn import CTC_Model
    model = CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=0.2)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return model.eval()


def test_drop_in_model_equals_hip_model():
    """models.cnn_rnn.CTC_Model.forward(x, x1) in eval mode is HipModel.forward bit for bit (x1 given or None, x on the host or the
    device); visualize=True returns the reference's four-element list; train mode raises NotImplementedError."""
    synth = _synth()
    geom = cc.geometry({})
    sd = synth.synth_state_dict(geom, seed=81)
    x = cc.draw_batch(geom, 3, 14, seed=82)
    want = _model(geom, sd, None).forward(_cuda(x), None, sync_errors=True).cpu().numpy()
    model = _drop_in(geom, sd)
    x1 = torch.ones((3, 4), dtype=torch.int64)
    got = model(torch.from_numpy(x), x1)
    assert not got.is_cuda
    np.testing.assert_array_equal(got.numpy(), want)
    np.testing.assert_array_equal(model(_cuda(x), None).cpu().numpy(), want)
    out, visual = model(torch.from_numpy(x), x1, visualize=True)
    np.testing.assert_array_equal(out.numpy(), want)
    assert len(visual) == 4 and visual[0].shape == (3, 14, geom.feat) and visual[1].shape == (3, geom.channels, 7, geom.w2)
    assert visual[2].shape == (7, 3, geom.rnn_in) and visual[3] is out
    taps = {}
    cc.forward_f64(sd, x, taps=taps)
    assert float(np.abs(visual[2].numpy() - taps["conv1"]).max()) <= cc.TOL
    model.train()
    with pytest.raises(NotImplementedError, match="CTC-only training is not built"):
        model(torch.from_numpy(x), x1)


# ----------------------------------------------------------------------------- infer
def test_infer_main_on_a_ctc_only_checkpoint(tmp_path, capsys):
    """The infer program over tests/golden/vocabulary_single with a save_package checkpoint of the CTC-only class, --timestamps
    --posteriors: load_model picks models.cnn_rnn, one block per word the dictionary holds, and the decoded sequences are the beam decode
    of HipModel.forward on the same batches."""
    from ctc_attention_mispronunciation_amd import infer as infer_mod
    from ctc_attention_mispronunciation_amd import infer_core
    from ctc_attention_mispronunciation_amd.dict.phonetic_dict import Phonetic
    from ctc_attention_mispronunciation_amd.models import cnn_rnn
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    from ctc_attention_mispronunciation_amd.utils.data_loader import Vocab, WavBatchLoader
    import types
    synth = _synth()
    data = tmp_path / "words"
    shutil.copytree(os.path.join(GOLD, "vocabulary_single"), str(data))
    i2c = synth.phone_table_41()
    (tmp_path / "units").write_text("".join(i2c[i] + "\n" for i in range(2, len(i2c))))
    geom = cc.geometry({})
    sd = synth.synth_state_dict(geom, seed=11)
    model = _drop_in(geom, sd)
    os.makedirs(str(tmp_path / "ckpt" / "exp"))
    torch.save(cnn_rnn.CTC_Model.save_package(model), str(tmp_path / "ckpt" / "exp" / "ctc_best_model.pkl"))
    arpa, cmvn_path, cmudict = os.path.join(GOLD, "lm_synth45.arpa"), os.path.join(GOLD, "global_fbank_cmvn.txt"), os.path.join(GOLD, "cmudict_subset.dict")
    conf = tmp_path / "conf.yaml"
    conf.write_text("exp_name: 'exp'\ncheckpoint_dir: '%s'\nvocab_file: '%s'\nleft_ctx: 0\nright_ctx: 2\nn_skip_frame: 2\n"
                    "n_downsample: 2\nbatch_size: 8\ndecode_type: 'Beam'\nbeam_width: 10\nlm_path: '%s'\nlm_alpha: 0\n"
                    % (tmp_path / "ckpt", tmp_path / "units", arpa))
    opts = types.SimpleNamespace(checkpoint_dir=str(tmp_path / "ckpt"), exp_name="exp")
    loaded = infer_mod.load_model(opts)
    assert type(loaded) is cnn_rnn.CTC_Model and not loaded.training and "embeds.weight" not in loaded.state_dict()
    seq = tmp_path / "decode_seq.txt"
    capsys.readouterr()
    assert infer_mod.main(["--conf", str(conf), "--wav_transcript_path", str(data), "--cmvn", cmvn_path, "--cmudict", cmudict,
                           "--decode_seq", str(seq), "--timestamps", "--posteriors"]) == 0
    stdout = capsys.readouterr().out
    assert stdout.count("id     : ") == 18
    for line in ("time   :", "gop    :", "post   :", "score  :"):
        assert stdout.count("\n" + line) == 18, line
    # the same batches through HipModel.forward and the beam decoder
    phonetic = Phonetic(cmudict)
    buf = io.StringIO()
    items, _, _, _ = infer_mod.collect(str(data), phonetic)
    vocab = Vocab(str(tmp_path / "units"))
    loader = WavBatchLoader(items, vocab, 8, cmvn=fb.cmvn_scale_offset(fb.read_cmvn_stats(cmvn_path)), right_ctx=2, n_skip_frame=2, n_downsample=2)
    decoder = BeamDecoder(vocab.index2word, beam_width=10, blank_index=0, space_idx=-1, lm_path=arpa, lm_alpha=0)
    hip = _model(geom, sd, None)
    for inputs, input_sizes, _, _, trans, trans_sizes, utts in loader:
        logp = hip.forward(inputs.to("cuda", torch.float32).contiguous(), None, sync_errors=True)
        lens = infer_core.frames_from_fraction(input_sizes, logp.size(0)).numpy().tolist()
        decoded = decoder.decode(logp, lens)
        trans, trans_sizes = trans.cpu().numpy(), trans_sizes.numpy()
        for b, utt in enumerate(utts):
            canonical = " ".join(vocab.index2word[n] for n in trans[b][:trans_sizes[b]])
            buf.write(utt + " " + " ".join(infer_core.diagnose(decoded[b], canonical, decoder, None)["decoded"]) + "\n")
    assert seq.read_text() == buf.getvalue() and len(buf.getvalue().splitlines()) == 18
    hip.close()
