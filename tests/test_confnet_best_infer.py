"""infer --joint_diagnosis end to end (GPU): the program's main() in this process, set up as tests/test_confnet_infer.py sets it up.  With
the flag every line of the flag-less output is unchanged and each block gains exactly one 'jdiag  :' line -- ``joint_diagnosis``' result on
the same posteriors through ``joint_diagnosis_line`` -- directly behind 'jpost' / 'post' and in front of 'nbest' / 'pron'; with
--timestamps a 'jtime  :' line follows it; with --pronunciations the lines are the chosen candidate's; the CTC-only checkpoint runs too."""
import contextlib
import io
import os
import re
import shutil

import pytest
import torch

from tests import ctc_only_cases as cc
from tests.helpers import GOLD
from tests.test_candidates import _blocks, _run_infer
from tests.test_nbest_infer import _setup, _stable

pytestmark = pytest.mark.gpu
P = ["--error_prior", "0.05"]
JDIAG = re.compile(r"^jdiag  : (\S+( \S+)*) \| edits (\d+) \| score (-?\d+\.\d{4}) \| p ([01]\.\d{4})$")
JTIME = re.compile(r"^jtime  : (\S+ \d+\.\d\d-\d+\.\d\d( |$))*$")


def test_infer_joint_diagnosis_end_to_end(tmp_path, monkeypatch):
    from ctc_attention_mispronunciation_amd import infer as infer_cli
    from ctc_attention_mispronunciation_amd.dict.phonetic_dict import Phonetic
    from ctc_attention_mispronunciation_amd.hip_model import ctc_variants
    from ctc_attention_mispronunciation_amd.infer_core import joint_diagnosis_line, joint_time_line, seconds_per_frame
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import joint_diagnosis
    from ctc_attention_mispronunciation_amd.utils.data_loader import Vocab, WavBatchLoader, frames_from_fraction
    monkeypatch.delenv("MDD_PRECISION", raising=False)
    model, i2c, arpa = _setup(tmp_path)
    plain = _run_infer(tmp_path, [])
    flagged = _run_infer(tmp_path, ["--joint_diagnosis"] + P)
    assert "jdiag  : " not in plain and "jtime  : " not in flagged
    # without its jdiag lines the output is the plain run's, byte for byte (the lines that print the run's folder or a timing apart)
    assert [line for line in _stable(flagged, tmp_path) if not line.startswith("jdiag  : ")] == _stable(plain, tmp_path)
    before, after = _blocks(plain), _blocks(flagged)
    assert sorted(before) == sorted(after) and len(after) == 18

    # joint_diagnosis on the same posteriors: the batch WavBatchLoader forms, one plain forward per candidate set
    with contextlib.redirect_stdout(io.StringIO()):
        vocab = Vocab(str(tmp_path / "units"))
        items, word_dict, transcripts, _ = infer_cli.collect(str(tmp_path / "words"), Phonetic(os.path.join(GOLD, "cmudict_subset.dict")), True)
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt")))
    loader = WavBatchLoader(items, vocab, 64, cmvn=cmvn, pronunciations=True)
    batches = list(loader)
    assert len(batches) == 1
    inputs, input_sizes, _, _, trans, trans_sizes, utts, cand = batches[0]
    per_set = []
    for ids, sizes in cand["sets"]:
        probs = model(inputs, ids.cuda())
        lens = frames_from_fraction(input_sizes, probs.size(0)).numpy().tolist()
        base = ctc_variants(probs, lens, ids.to(torch.int32), sizes.to(torch.int32), 0, want_ins=False).base.cpu().tolist()
        spf = seconds_per_frame(loader, inputs.size(1) // probs.size(0))
        per_set.append(dict(ids=ids.numpy(), sizes=sizes.numpy(), base=base, diag=joint_diagnosis(probs, lens, ids.cuda(), sizes, 0, error_prior=0.05)))

    def want_lines(k, x):
        s = per_set[k]
        diag = s["diag"][x]
        assert diag is not None and len(diag[0]) == s["sizes"][x] and len(diag[1]) == s["sizes"][x] + 1 and 0.0 < diag[3] <= 1.0
        own = s["ids"][x][:s["sizes"][x]]
        return joint_diagnosis_line(diag, own, vocab.index2word, 0), joint_time_line(diag, vocab.index2word, spf, 0)

    for x, u in enumerate(utts):
        assert after[u][:12] == before[u][:12] and len(after[u]) == 13, u          # one line behind 'score  :', nothing else
        assert after[u][12] == want_lines(0, x)[0] and JDIAG.match(after[u][12]), (u, after[u][12])

    # with every other line: behind post and jpost, in front of nbest and pron, jtime behind jdiag, and the chosen candidate's
    rest = ["--timestamps", "--posteriors", "--pronunciations", "--nbest", "2", "--joint_posteriors"] + P
    base_t, with_t = _blocks(_run_infer(tmp_path, rest)), _blocks(_run_infer(tmp_path, rest + ["--joint_diagnosis"]))
    moved = 0
    for x, u in enumerate(utts):
        assert [line for line in with_t[u] if not line.startswith(("jdiag  : ", "jtime  : "))] == base_t[u], u
        assert [line[:9] for line in with_t[u][12:]] == ["time   : ", "gop    : ", "post   : ", "jpost  : ", "jdiag  : ", "jtime  : ", "nbest  : ",
                                                         "nbest  : ", "pron   : "], u
        n = cand["counts"][x]
        ll = [per_set[k]["base"][x] for k in range(n)]
        chosen = max(range(n), key=lambda k: (ll[k], -k))
        assert (with_t[u][16], with_t[u][17]) == want_lines(chosen, x), (u, chosen)
        assert JTIME.match(with_t[u][17]), with_t[u][17]
        moved += chosen != 0
    assert moved >= 1, "no utterance chose a later pronunciation: the candidate's own lines went unchecked"


def test_infer_joint_diagnosis_on_a_ctc_only_checkpoint(tmp_path, capsys):
    from ctc_attention_mispronunciation_amd import infer as infer_mod
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.models import cnn_rnn
    from tests.test_ctc_only import _drop_in
    data = tmp_path / "words"
    shutil.copytree(os.path.join(GOLD, "vocabulary_single"), str(data))
    i2c = synth.phone_table_41()
    (tmp_path / "units").write_text("".join(i2c[i] + "\n" for i in range(2, len(i2c))))
    geom = cc.geometry({})
    model = _drop_in(geom, synth.synth_state_dict(geom, seed=11))
    os.makedirs(str(tmp_path / "ckpt" / "exp"))
    torch.save(cnn_rnn.CTC_Model.save_package(model), str(tmp_path / "ckpt" / "exp" / "ctc_best_model.pkl"))
    arpa, cmvn_path, cmudict = os.path.join(GOLD, "lm_synth45.arpa"), os.path.join(GOLD, "global_fbank_cmvn.txt"), os.path.join(GOLD, "cmudict_subset.dict")
    conf = tmp_path / "conf.yaml"
    conf.write_text("exp_name: 'exp'\ncheckpoint_dir: '%s'\nvocab_file: '%s'\nleft_ctx: 0\nright_ctx: 2\nn_skip_frame: 2\n"
                    "n_downsample: 2\nbatch_size: 8\ndecode_type: 'Beam'\nbeam_width: 10\nlm_path: '%s'\nlm_alpha: 0\n"
                    % (tmp_path / "ckpt", tmp_path / "units", arpa))
    capsys.readouterr()
    assert infer_mod.main(["--conf", str(conf), "--wav_transcript_path", str(data), "--cmvn", cmvn_path, "--cmudict", cmudict,
                           "--timestamps", "--joint_diagnosis"] + P) == 0
    lines = capsys.readouterr().out.split("\n")
    diag = [line for line in lines if line.startswith("jdiag  : ")]
    times = [line for line in lines if line.startswith("jtime  : ")]
    assert len(diag) == 18 and len(times) == 18
    assert all(JDIAG.match(line) for line in diag), [line for line in diag if not JDIAG.match(line)][:3]
    for n, line in enumerate(lines):
        if line.startswith("jdiag  : "):
            assert lines[n - 1].startswith("gop    : ") and lines[n + 1].startswith("jtime  : ") and lines[n + 2] == "", line
