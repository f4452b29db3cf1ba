"""Batch inference (AA/infer.py's loop and driver): the one-launch batched fbank front end (mdd_fbank_batch / fbank_batch), the
``infer`` mirror and ``WavBatchLoader`` against G13 (the reference's own ``infer()`` over a padded batch, tools/gen_golden_infer.py),
and the command-line driver end to end."""
import hashlib
import io
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests.helpers import GOLD, ROOT, jload, npz

TOL = 1e-4
TOL_ORACLE = 2e-5       # tests/test_oracle.py
VOCAB_DIR = os.path.join(GOLD, "vocabulary_single")


def _lib():
    from ctc_attention_mispronunciation_amd import _lib
    return _lib.lib()


def _read_wav(i):
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    wav, rate = fb.read_wav(os.path.join(VOCAB_DIR, "%d.wav" % i))
    assert rate == 16000
    return wav


def _g13_batches(meta, bs):
    """G13's utterances of one case as the package's create_input batches of the oracle's features (the golden's own inputs)."""
    from oracle import oracle as orc
    from ctc_attention_mispronunciation_amd.synth import phone_table_41
    from ctc_attention_mispronunciation_amd.utils.data_loader import create_input
    c2i = {v: k for k, v in phone_table_41().items()}
    stats = orc.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt"))
    order = meta["order"]
    batches = []
    for s in range(0, len(order), bs):
        items = []
        for u in order[s:s + bs]:
            feats = orc.stack_skip(orc.apply_cmvn(orc.fbank(_read_wav(int(u))), stats))
            assert feats.shape[0] == meta["utts"][u]["T"]
            ids = torch.LongTensor([c2i[p] for p in meta["utts"][u]["canonical"].split()])
            items.append((torch.from_numpy(feats), ids, ids, u))
        batches.append(create_input(items))
    return batches


def _case(meta, bs):
    return [c for c in meta["cases"] if c["batch_size"] == bs][0]


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_fbank_batch_len_matches_per_utterance_lengths():
    import ctypes as C
    L = _lib()
    T_raw = lambda n: L.mdd_fbank_num_frames(n)   # noqa: E731
    lens = [400, 401, 559, 560, 400 + 160 * 4, 400 + 160 * 5, 160000]
    assert T_raw(400) == 1 and T_raw(559) == 1 and T_raw(560) == 2 and T_raw(1040) == 5 and T_raw(1200) == 6
    for skip, n_down in ((2, 2), (1, 2), (3, 4), (2, 1)):
        for subset in [[n] for n in lens] + [lens, lens[:4], lens[2:6]]:
            a = np.array(subset, dtype=np.int64)
            got = L.mdd_fbank_batch_len(a.ctypes.data_as(C.POINTER(C.c_int64)), len(a), skip, n_down)
            assert got == max(L.mdd_stack_len(T_raw(int(n)), skip, n_down) for n in subset), (subset, skip, n_down)
    a = np.array([400, 160000, 399, 1040], dtype=np.int64)
    assert L.mdd_fbank_batch_len(a.ctypes.data_as(C.POINTER(C.c_int64)), 4, 2, 2) == -1
    assert "utterance 2" in L.mdd_last_error().decode()


def test_fbank_batch_rejects_bad_arguments():
    """Argument checks happen before any device work: B <= 0, one CMVN pointer without the other, right < 0, skip < 1."""
    import ctypes as C
    L = _lib()
    host = np.zeros(81, np.float32)    # a real (host) address; every call below is refused before any pointer is used
    buf = C.c_void_p(host.ctypes.data)
    for B, sc, of, right, skip in ((0, None, None, 2, 2), (-1, None, None, 2, 2), (2, buf, None, 2, 2), (2, None, buf, 2, 2),
                                   (2, None, None, -1, 2), (2, None, None, 2, 0)):
        assert L.mdd_fbank_batch(buf, buf, B, 10, sc, of, right, skip, 2, buf, None) == -1, (B, sc, of, right, skip)


def test_fbank_batch_raises_value_error_naming_the_short_utterance():
    """The length check comes before any device work."""
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    with pytest.raises(ValueError, match="utterance 2 is shorter than one 400-sample window"):
        fb.fbank_batch([np.zeros(1000, np.float32), np.zeros(400, np.float32), np.zeros(399, np.float32)])


def test_g13_integrity_against_ref_port():
    """G13's log-probs and input_sizes come back from the package's create_input batches of the oracle features through
    oracle.ref_port (the torch restatement of the reference graph) -- for every batch of both cases."""
    from oracle import ref_port
    from ctc_attention_mispronunciation_amd import synth
    meta, g = jload("g13_infer.json"), npz("g13_infer.npz")
    assert len(meta["order"]) == 18 and meta["order"] == sorted(meta["order"])
    sd = synth.synth_state_dict(synth.Geometry(**synth.REFERENCE), seed=11)
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    for bs in (64, 8):
        case = _case(meta, bs)
        batches = _g13_batches(meta, bs)
        assert len(batches) == len(case["batches"]) == (1 if bs == 64 else 3)
        for k, (b, rec) in enumerate(zip(batches, case["batches"])):
            inputs, sizes, _, _, trans, _, utts = b
            assert utts == rec["utts"] and inputs.shape[1] == rec["T_max"] and trans.shape[1] == rec["L_max"]
            np.testing.assert_array_equal(sizes.numpy(), g["bs%d_b%d_input_sizes" % (bs, k)])
            lp = ref_port.forward(sd, inputs.numpy(), trans.numpy()).numpy()
            np.testing.assert_allclose(lp, g["bs%d_b%d_logp" % (bs, k)], rtol=0, atol=TOL_ORACLE)


def _cli(args, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "ctc_attention_mispronunciation_amd.infer"] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("flags,needs", [(["-p", "g2p"], "g2p_en"), (["-p", "phonemizer"], "phonemizer"),
                                         (["-p", "transcript"], "textgrid"), (["-f", "ipa"], "phonemizer")])
def test_cli_refuses_what_needs_absent_dependencies(tmp_path, flags, needs):
    r = _cli(["--conf", str(tmp_path / "none.yaml"), "--wav_transcript_path", str(tmp_path)] + flags, timeout=120)
    assert r.returncode == 2, (r.stdout, r.stderr)
    assert needs in r.stderr and "not available offline" in r.stderr
    assert os.listdir(str(tmp_path)) == []


# ------------------------------------------------------------------------------------------------------------------- GPU
def _per_utterance_batch(wavs, cmvn):
    """compute_fbank_feats -> stack_features -> create_input: the per-utterance route to the padded batch."""
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.data_loader import create_input, stack_features
    one = torch.LongTensor([1])
    items = [(stack_features(fb.compute_fbank_feats(w, cmvn=cmvn)).cpu(), one, one, "u%d" % i) for i, w in enumerate(wavs)]
    return create_input(items)


def _synthetic_wavs():
    rs = np.random.default_rng(7)
    lens = [400,                 # exactly one window
            400 + 160 * 4,       # T_raw 5 -> 3 kept rows -> the even-pad row
            400 + 160 * 5, 559, 12345,
            160000]              # 10 s
    return [(rs.standard_normal(n) * 3000).astype(np.float32) for n in lens]


@pytest.mark.gpu
@pytest.mark.parametrize("use_cmvn", [True, False])
def test_fbank_batch_bit_identical_to_per_utterance_route(use_cmvn):
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt"))) if use_cmvn else None
    vocab = [_read_wav(i) for i in range(1, 21)]
    syn = _synthetic_wavs()
    for wavs in (vocab, syn, syn[::-1], vocab[:7] + syn, [syn[-1]], [syn[0]], [vocab[3]]):
        want_x, want_s = _per_utterance_batch(wavs, cmvn)[:2]
        out = torch.full(tuple(want_x.shape), float("nan"), dtype=torch.float32, device="cuda")
        x, s = fb.fbank_batch(wavs, cmvn=cmvn, out=out)
        torch.cuda.synchronize()
        assert x.data_ptr() == out.data_ptr()
        assert s.dtype == torch.float32 and s.device.type == "cpu"
        assert torch.equal(x.cpu(), want_x), float((x.cpu() - want_x).abs().nan_to_num(1e30).max())
        assert torch.equal(s, want_s)
        x2, s2 = fb.fbank_batch(wavs, cmvn=cmvn)                # torch.empty output: written whole as well
        assert torch.equal(x2.cpu(), want_x) and torch.equal(s2, want_s)


@pytest.mark.gpu
def test_fbank_batch_equals_reference_shaped_route(tmp_path):
    """WAV -> write_ark_scp -> SpeechDataset -> SpeechDataLoader(batch_size=64, shuffle=False): the reference's route through
    disk and host numpy; the one-launch batch gives the same inputs and input_sizes."""
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.data_loader import SpeechDataLoader, SpeechDataset, Vocab
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt")))
    wavs = [_read_wav(i) for i in range(1, 21)] + _synthetic_wavs()
    utts = ["u%02d" % i for i in range(len(wavs))]
    fb.write_ark_scp(str(tmp_path / "fbank.ark"), str(tmp_path / "fbank.scp"),
                     {u: fb.compute_fbank_feats(w, cmvn=cmvn) for u, w in zip(utts, wavs)})
    (tmp_path / "units").write_text("sil\n")
    (tmp_path / "trans").write_text("".join("%s sil\n" % u for u in utts))
    opts = types.SimpleNamespace(left_ctx=0, right_ctx=2, n_skip_frame=2, n_downsample=2)
    ds = SpeechDataset(Vocab(str(tmp_path / "units")), str(tmp_path / "fbank.scp"), str(tmp_path / "trans"),
                       str(tmp_path / "trans"), opts)
    batches = list(SpeechDataLoader(ds, batch_size=64, shuffle=False))
    assert len(batches) == 1 and batches[0][6] == utts
    x, s = fb.fbank_batch(wavs, cmvn=cmvn)
    assert torch.equal(x.cpu(), batches[0][0])
    assert torch.equal(s, batches[0][1])


class _CapturingModel(object):
    def __init__(self, hip):
        self.hip, self.outputs = hip, []

    def __call__(self, inputs, trans):
        lp = self.hip.forward(inputs.to("cuda", torch.float32).contiguous(), trans.to("cuda", torch.int64).contiguous(),
                              sync_errors=True)
        self.outputs.append(lp.cpu().numpy())
        return lp


def _top2_gaps(lp, sizes, utts, bad):
    """Smallest top-2 log-prob gap over the counted frames of each utterance in `bad` (what the diagnosis of a mismatch needs)."""
    T = lp.shape[0]
    out = {}
    for b, u in enumerate(utts):
        if u in bad:
            n = int(np.float32(sizes[b]) * np.float32(T))
            top = np.sort(lp[:n, b, :], axis=-1)
            out[u] = float((top[:, -1] - top[:, -2]).min())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("bs", [64, 8])
@pytest.mark.parametrize("precision", ["f32x6", "f32", "bf16x3"])
def test_infer_matches_reference_infer(tmp_path, precision, bs):
    """The infer mirror against G13 (the reference's own infer()), (a) on G13's own features through create_input, (b) from the
    WAVs through WavBatchLoader (fbank_batch): log-probs of every batch within 1e-4; stdout, decode_seq lines and totals identical."""
    from tests.helpers import record_margin
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    from ctc_attention_mispronunciation_amd.infer_core import infer
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    from ctc_attention_mispronunciation_amd.utils.data_loader import WavBatchLoader
    meta, g = jload("g13_infer.json"), npz("g13_infer.npz")
    case = _case(meta, bs)
    geom = synth.Geometry(**synth.REFERENCE)
    hip = HipModel(geom, synth.synth_state_dict(geom, seed=11), precision=precision)
    assert hip.precision == precision
    i2c = synth.phone_table_41()
    vocab = types.SimpleNamespace(index2word=i2c, word2index={v: k for k, v in i2c.items()})
    beam = BeamDecoder(i2c, beam_width=10, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=0.0)
    phonetic = types.SimpleNamespace(api_word_translation=lambda utterance: "")
    word_dict = {u: {"ipa": meta["utts"][u]["cmu"]} for u in meta["order"]}
    words = {u: meta["utts"][u]["word"] for u in meta["order"]}
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt")))
    routes = {"g13feats": _g13_batches(meta, bs),
              "wav": WavBatchLoader([(u, _read_wav(int(u)), meta["utts"][u]["canonical"]) for u in meta["order"]], vocab, bs, cmvn)}
    for route, loader in routes.items():
        model = _CapturingModel(hip)
        buf = io.StringIO()
        seq = str(tmp_path / ("%s_decode_seq.txt" % route))
        totals = infer(phonetic, word_dict, loader, torch.device("cuda"), model, beam, vocab, words, False, out=buf,
                       decode_seq_path=seq)
        assert len(model.outputs) == len(case["batches"])
        worst = 0.0
        for k, lp in enumerate(model.outputs):
            ref = g["bs%d_b%d_logp" % (bs, k)]
            assert lp.shape == ref.shape, (route, k)
            worst = max(worst, float(np.abs(lp - ref).max()))
        record_margin("g13_bs%d_%s_%s_logp" % (bs, route, precision), worst, TOL)
        assert worst <= TOL, (route, worst)
        got, want = buf.getvalue(), case["stdout"]
        if got != want:
            gb, wb = got.split("id     : "), want.split("id     : ")
            bad = {w.split("\n")[0] for a, w in zip(gb, wb) if a != w}
            gaps = {}
            for k, rec in enumerate(case["batches"]):
                gaps.update(_top2_gaps(model.outputs[k], g["bs%d_b%d_input_sizes" % (bs, k)], rec["utts"], bad))
            raise AssertionError("%s %s bs=%d: blocks differ for %s (smallest top-2 gaps %s)" % (route, precision, bs, sorted(bad), gaps))
        assert open(seq).read().splitlines() == case["decode_seq"]
        assert list(totals) == case["totals"]


def _tree_digest(path):
    h = hashlib.sha256()
    for name in sorted(os.listdir(path)):
        h.update(name.encode())
        with open(os.path.join(path, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


@pytest.mark.gpu
def test_cli_end_to_end(tmp_path):
    """python -m ctc_attention_mispronunciation_amd.infer over a copy of vocabulary_single with a save_package checkpoint of the
    seed-11 weights: exit 0, the per-utterance blocks are G13's batch_size=64 output, the two words the dictionary lacks are
    skipped with a line each, and the input folder is left as it was."""
    import shutil
    import torch.nn as nn
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    from ctc_attention_mispronunciation_amd.utils.data_loader import Vocab
    data = tmp_path / "words"
    shutil.copytree(VOCAB_DIR, str(data))
    before = _tree_digest(str(data))
    i2c = synth.phone_table_41()
    (tmp_path / "units").write_text("".join(i2c[i] + "\n" for i in range(2, len(i2c))))
    assert Vocab(str(tmp_path / "units")).index2word == i2c
    geom = synth.Geometry(**synth.REFERENCE)
    model = CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=0.2)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(geom, seed=11).items()})
    os.makedirs(str(tmp_path / "ckpt" / "exp"))
    torch.save(CTC_Model.save_package(model), str(tmp_path / "ckpt" / "exp" / "ctc_best_model.pkl"))
    conf = tmp_path / "conf.yaml"
    conf.write_text("exp_name: 'exp'\ncheckpoint_dir: '%s'\nvocab_file: '%s'\nleft_ctx: 0\nright_ctx: 2\nn_skip_frame: 2\n"
                    "n_downsample: 2\nbatch_size: 64\ndecode_type: 'Beam'\nbeam_width: 10\nlm_path: '%s'\nlm_alpha: 0\n"
                    % (tmp_path / "ckpt", tmp_path / "units", os.path.join(GOLD, "lm_synth45.arpa")))
    r = _cli(["--conf", str(conf), "--wav_transcript_path", str(data), "--cmvn", os.path.join(GOLD, "global_fbank_cmvn.txt"),
              "--cmudict", os.path.join(GOLD, "cmudict_subset.dict")], timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    want = _case(jload("g13_infer.json"), 64)
    assert want["stdout"] in r.stdout, r.stdout
    assert "12 skipped: 'OPPO' is not in the CMU dictionary" in r.stdout
    assert "17 skipped: 'longtimenosee' is not in the CMU dictionary" in r.stdout
    assert "%d %d %d" % tuple(want["totals"]) in r.stdout and "RTF: " in r.stdout
    assert _tree_digest(str(data)) == before


@pytest.mark.gpu
@pytest.mark.parametrize("T_raw", [1000, 997, 7])
def test_forward_raw_f32x6_equals_stack_then_forward(T_raw):
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    from ctc_attention_mispronunciation_amd.utils.data_loader import stack_features
    geom = synth.Geometry(**synth.REFERENCE)
    raw = torch.from_numpy(synth.synth_raw_features(3, T_raw, 81, seed=T_raw)).cuda()
    _, x1, _, _ = synth.synth_batch(geom, B=3, T=max(2, T_raw // 2 * 2), L=5, seed=1, ragged=False)
    x1 = torch.from_numpy(np.ascontiguousarray(x1)).cuda()
    m = HipModel(geom, synth.synth_state_dict(geom, seed=5), precision="f32x6")
    assert m.precision == "f32x6"
    want = m.forward(stack_features(raw), x1, sync_errors=True).cpu().numpy()
    got = m.forward_raw(raw, x1, sync_errors=True).cpu().numpy()
    np.testing.assert_array_equal(got, want)
