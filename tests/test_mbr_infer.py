"""infer --mbr N end to end (GPU): the program's main() in this process over the synthetic-checkpoint folder of tests/test_nbest_infer.py.
With --mbr 5 every block gains exactly one 'mbr    :' line -- ``decode_mbr``'s record on the same posteriors through ``mbr_line`` -- behind
the 'nbest' lines and in front of 'pron'; with those lines removed the output is the output without the flag, byte for byte; it holds
beside --nbest 3 --timestamps --posteriors, with --pronunciations the line is the chosen candidate's, and the CTC-only checkpoint runs too."""
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
N = 5
LINE = re.compile(r"^mbr    : ([1-5]) (\S+( \S+)*) \| risk (\d+\.\d{4}) \| risk1 (\d+\.\d{4}) \| exp (\d+\.\d{4}) \| Comp\. (\d+)/(\d+)$")


def test_infer_mbr_end_to_end(tmp_path, monkeypatch):
    from ctc_attention_mispronunciation_amd import infer as infer_cli
    from ctc_attention_mispronunciation_amd.dict.phonetic_dict import Phonetic
    from ctc_attention_mispronunciation_amd.hip_model import ctc_variants
    from ctc_attention_mispronunciation_amd.infer_core import mbr_line
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    from ctc_attention_mispronunciation_amd.utils.data_loader import Vocab, WavBatchLoader, frames_from_fraction
    monkeypatch.delenv("MDD_PRECISION", raising=False)
    model, i2c, arpa = _setup(tmp_path)
    plain = _run_infer(tmp_path, [])
    flagged = _run_infer(tmp_path, ["--mbr", str(N)])
    assert "mbr    : " not in plain
    # without its mbr lines the output is the plain run's, byte for byte (the lines that print the run's folder or a timing apart)
    assert [line for line in _stable(flagged, tmp_path) if not line.startswith("mbr    : ")] == _stable(plain, tmp_path)
    before, after = _blocks(plain), _blocks(flagged)
    assert sorted(before) == sorted(after) and len(after) == 18

    # decode_mbr on the same posteriors: the batch WavBatchLoader forms, one plain forward per candidate set
    with contextlib.redirect_stdout(io.StringIO()):
        vocab = Vocab(str(tmp_path / "units"))
        items, word_dict, transcripts, _ = infer_cli.collect(str(tmp_path / "words"), Phonetic(os.path.join(GOLD, "cmudict_subset.dict")), True)
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt")))
    batches = list(WavBatchLoader(items, vocab, 64, cmvn=cmvn, pronunciations=True))
    assert len(batches) == 1
    inputs, input_sizes, _, _, trans, trans_sizes, utts, cand = batches[0]
    beam = BeamDecoder(i2c, beam_width=10, blank_index=0, space_idx=-1, lm_path=arpa, lm_alpha=0.0)
    per_set = []
    for ids, sizes in cand["sets"]:
        probs = model(inputs, ids.cuda())
        lens = frames_from_fraction(input_sizes, probs.size(0)).numpy().tolist()
        base = ctc_variants(probs, lens, ids.to(torch.int32), sizes.to(torch.int32), 0, want_ins=False).base.cpu().tolist()
        per_set.append(dict(ids=ids.numpy(), sizes=sizes.numpy(), base=base, mbr=beam.decode_mbr(probs, lens, N, ids.cuda(), sizes),
                            decoded=beam.decode(probs, lens), nbest=beam.decode_nbest(probs, lens, N, rescore=False)))

    def want_line(k, x):
        s = per_set[k]
        canonical = " ".join(i2c[i] for i in s["ids"][x][:s["sizes"][x]])
        return mbr_line(s["mbr"][x], canonical, beam)

    for x, u in enumerate(utts):
        assert after[u][:12] == before[u][:12] and len(after[u]) == 13, u          # one line behind 'score  :', nothing else
        assert after[u][12] == want_line(0, x), (u, after[u][12])
        m = LINE.match(after[u][12])
        assert m, after[u][12]
        rec = per_set[0]["mbr"][x]
        assert int(m.group(1)) == rec[1] + 1 and m.group(2) == rec[0] == per_set[0]["nbest"][x][rec[1]][0], u
        assert float(m.group(4)) <= float(m.group(5)) + 1e-4                        # the MBR hypothesis' risk is the least among the ranks that count
        if rec[1] == 0:
            assert m.group(2) == per_set[0]["decoded"][x] and m.group(4) == m.group(5)
            assert ("Comp.  : %s/%s" % m.groups()[-2:]) == after[u][10], u           # rank 1's Comp. is the block's own

    # with the other lines: behind time / gop / post / nbest and in front of pron, the chosen candidate's
    rest = ["--nbest", "3", "--timestamps", "--posteriors"]
    base_t, with_t = _blocks(_run_infer(tmp_path, rest)), _blocks(_run_infer(tmp_path, rest + ["--mbr", str(N)]))
    for x, u in enumerate(utts):
        assert [line for line in with_t[u] if not line.startswith("mbr    : ")] == base_t[u], u
        assert [line[:9] for line in with_t[u][12:]] == ["time   : ", "gop    : ", "post   : "] + ["nbest  : "] * 3 + ["mbr    : "], u
        assert with_t[u][18] == want_line(0, x), u
    rest = rest + ["--pronunciations"]
    base_t, with_t = _blocks(_run_infer(tmp_path, rest)), _blocks(_run_infer(tmp_path, rest + ["--mbr", str(N)]))
    moved = 0
    for x, u in enumerate(utts):
        assert [line for line in with_t[u] if not line.startswith("mbr    : ")] == base_t[u], u
        assert [line[:9] for line in with_t[u][12:]] == ["time   : ", "gop    : ", "post   : "] + ["nbest  : "] * 3 + ["mbr    : ", "pron   : "], u
        n = cand["counts"][x]
        ll = [per_set[k]["base"][x] for k in range(n)]
        chosen = max(range(n), key=lambda k: (ll[k], -k))
        assert with_t[u][18] == want_line(chosen, x), (u, chosen)
        moved += chosen != 0
    assert moved >= 1, "no utterance chose a later pronunciation: the candidate's own line went unchecked"


def test_infer_mbr_on_a_ctc_only_checkpoint(tmp_path, capsys):
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
    args = ["--conf", str(conf), "--wav_transcript_path", str(data), "--cmvn", cmvn_path, "--cmudict", cmudict]
    assert infer_mod.main(args) == 0
    plain = capsys.readouterr().out
    assert infer_mod.main(args + ["--mbr", str(N)]) == 0
    lines = capsys.readouterr().out.split("\n")
    got = [line for line in lines if line.startswith("mbr    : ")]
    assert len(got) == 18 and all(LINE.match(line) for line in got), [line for line in got if not LINE.match(line)][:3]
    assert _stable("\n".join(line for line in lines if not line.startswith("mbr    : ")), tmp_path) == _stable(plain, tmp_path)
    for n, line in enumerate(lines):
        if line.startswith("mbr    : "):
            assert lines[n - 1].startswith("score  : ") and lines[n + 1] == "", line
