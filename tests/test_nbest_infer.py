"""infer --nbest N end to end (GPU): the program's main() in this process over tests/golden/vocabulary_single with cmudict_subset.dict and
the seed-11 H = 384 checkpoint -- the set-up of tests/test_infer_batch.py::test_cli_end_to_end, driven as tests/test_candidates.py drives
it.  With the 'nbest  :' lines removed the output is the output without the flag, byte for byte; every block has exactly N such lines in
rank order, rank 1 starred and carrying the block's decoded phones; score, loglik and p are decode_nbest's on the same posteriors; with
--pronunciations the lines are the chosen candidate's and sit in front of the 'pron' line."""
import contextlib
import io
import os
import re
import shutil

import pytest
import torch

from ctc_attention_mispronunciation_amd import synth
from tests.helpers import GOLD
from tests.test_candidates import TWO, _blocks, _run_infer, _torch_model, _volatile
from tests.test_infer_batch import VOCAB_DIR

pytestmark = pytest.mark.gpu
N = 3
LINE = re.compile(r"^nbest  : (\d+) ([* ]) (.*) \| score (\S+) \| loglik (\S+) \| p (\S+) \| Comp\. (\d+)/(\d+)$")


def _setup(tmp_path):
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    shutil.copytree(VOCAB_DIR, str(tmp_path / "words"))
    i2c = synth.phone_table_41()
    (tmp_path / "units").write_text("".join(i2c[i] + "\n" for i in range(2, len(i2c))))
    geom = synth.Geometry(**synth.REFERENCE)
    model = _torch_model(geom, synth.synth_state_dict(geom, seed=11))
    os.makedirs(str(tmp_path / "ckpt" / "exp"))
    torch.save(CTC_Model.save_package(model), str(tmp_path / "ckpt" / "exp" / "ctc_best_model.pkl"))
    arpa = os.path.join(GOLD, "lm_synth45.arpa")
    (tmp_path / "conf.yaml").write_text("exp_name: 'exp'\ncheckpoint_dir: '%s'\nvocab_file: '%s'\nleft_ctx: 0\nright_ctx: 2\nn_skip_frame: 2\n"
                                        "n_downsample: 2\nbatch_size: 64\ndecode_type: 'Beam'\nbeam_width: 10\nlm_path: '%s'\nlm_alpha: 0\n"
                                        % (tmp_path / "ckpt", tmp_path / "units", arpa))
    return model, i2c, arpa


def _stable(stdout, tmp_path):
    return [line for line in stdout.split("\n") if not _volatile(line, str(tmp_path))]


def _want_lines(records, canonical, beam):
    from ctc_attention_mispronunciation_amd.infer_core import diagnose
    out = []
    for n, (hyp, score, loglik, share) in enumerate(records):
        d = diagnose(hyp, canonical, beam)
        out.append((str(n + 1), "*" if n == 0 else " ", hyp, "%.4f" % score, "%.4f" % loglik, "%.4f" % share,
                    str(d["correct"]), str(d["correct"] + d["del_sub"])))
    return out


def test_infer_nbest_end_to_end(tmp_path, monkeypatch):
    from ctc_attention_mispronunciation_amd import infer as infer_cli
    from ctc_attention_mispronunciation_amd.dict.phonetic_dict import Phonetic
    from ctc_attention_mispronunciation_amd.hip_model import ctc_variants
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    from ctc_attention_mispronunciation_amd.utils.data_loader import Vocab, WavBatchLoader, frames_from_fraction
    monkeypatch.delenv("MDD_PRECISION", raising=False)
    model, i2c, arpa = _setup(tmp_path)
    plain = _run_infer(tmp_path, [])
    flagged = _run_infer(tmp_path, ["--nbest", str(N)])
    assert "nbest  : " not in plain
    # without its nbest lines the output is the plain run's, byte for byte (the lines that print the run's folder or a timing apart)
    assert [line for line in _stable(flagged, tmp_path) if not line.startswith("nbest  : ")] == _stable(plain, tmp_path)
    before, after = _blocks(plain), _blocks(flagged)
    assert sorted(before) == sorted(after) and len(after) == 18

    # decode_nbest on the same posteriors: the batch WavBatchLoader forms, one plain forward
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
        per_set.append((beam.decode_nbest(probs, lens, N), beam.decode(probs, lens), ids.numpy(), sizes.numpy(), base))

    def canonical(k, x):
        return " ".join(i2c[i] for i in per_set[k][2][x][:per_set[k][3][x]])

    for x, u in enumerate(utts):
        assert after[u][:12] == before[u][:12] and len(after[u]) == 12 + N, u          # N lines behind 'score  :', nothing else
        got = [LINE.match(line) for line in after[u][12:]]
        assert all(got), (u, after[u][12:])
        got = [m.groups() for m in got]
        assert got == _want_lines(per_set[0][0][x], canonical(0, x), beam), u
        assert [g[0] for g in got] == ["1", "2", "3"] and [g[1] for g in got] == ["*", " ", " "]
        assert got[0][2] == per_set[0][1][x]                                             # rank 1: the block's decoded phones
        assert ("Comp.  : %s/%s" % got[0][6:8]) == after[u][10], u                       # rank 1's Comp. is the block's own
        assert float(got[0][3]) >= float(got[1][3]) >= float(got[2][3])

    # with --pronunciations (and the other lines): the chosen candidate's list, behind time / gop / post and in front of pron
    both = ["--timestamps", "--posteriors", "--pronunciations"]
    base_t, with_t = _blocks(_run_infer(tmp_path, both)), _blocks(_run_infer(tmp_path, both + ["--nbest", str(N)]))
    words = {u: transcripts[u].strip().lower() for u in transcripts}
    moved = 0
    for x, u in enumerate(utts):
        assert [line for line in with_t[u] if not line.startswith("nbest  : ")] == base_t[u], u
        assert [line[:9] for line in with_t[u][12:]] == ["time   : ", "gop    : ", "post   : "] + ["nbest  : "] * N + ["pron   : "], u
        n = cand["counts"][x]
        ll = [per_set[k][4][x] for k in range(n)]
        chosen = max(range(n), key=lambda k: (ll[k], -k))
        got = [LINE.match(line).groups() for line in with_t[u][15:15 + N]]
        assert got == _want_lines(per_set[chosen][0][x], canonical(chosen, x), beam), (u, chosen)
        moved += chosen != 0
    assert moved >= 1 and TWO <= set(words.values()), "no utterance chose a later pronunciation: the candidate's own list went unchecked"
