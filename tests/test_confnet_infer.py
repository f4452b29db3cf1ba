"""infer --joint_posteriors end to end (GPU): the program's main() in this process, set up as tests/test_nbest_infer.py sets it up.  With
the flag every line of the flag-less output is unchanged and each block gains one 'jpost  :' line whose numbers are
``joint_phoneme_posteriors``' on the same posteriors; it sits directly behind 'post' and in front of 'nbest' / 'pron'; with
--pronunciations it is the chosen candidate's; --error_prior changes the numbers and nothing else."""
import contextlib
import io
import os

import pytest
import torch

from tests.helpers import GOLD
from tests.test_candidates import _blocks, _run_infer
from tests.test_nbest_infer import _setup, _stable

pytestmark = pytest.mark.gpu


def test_infer_joint_posteriors_end_to_end(tmp_path, monkeypatch):
    from ctc_attention_mispronunciation_amd import infer as infer_cli
    from ctc_attention_mispronunciation_amd.dict.phonetic_dict import Phonetic
    from ctc_attention_mispronunciation_amd.hip_model import ctc_variants
    from ctc_attention_mispronunciation_amd.infer_core import diagnose_posterior, posterior_line
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder, joint_phoneme_posteriors
    from ctc_attention_mispronunciation_amd.utils.data_loader import Vocab, WavBatchLoader, frames_from_fraction
    monkeypatch.delenv("MDD_PRECISION", raising=False)
    model, i2c, arpa = _setup(tmp_path)
    plain = _run_infer(tmp_path, [])
    flagged = _run_infer(tmp_path, ["--joint_posteriors"])
    assert "jpost  : " not in plain
    # without its jpost lines the output is the plain run's, byte for byte (the lines that print the run's folder or a timing apart)
    assert [line for line in _stable(flagged, tmp_path) if not line.startswith("jpost  : ")] == _stable(plain, tmp_path)
    before, after = _blocks(plain), _blocks(flagged)
    assert sorted(before) == sorted(after) and len(after) == 18

    # joint_phoneme_posteriors on the same posteriors: the batch WavBatchLoader forms, one plain forward per candidate set
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
        per_set.append(dict(decoded=beam.decode(probs, lens), ids=ids.numpy(), sizes=sizes.numpy(), base=base,
                            uniform=joint_phoneme_posteriors(probs, lens, ids.cuda(), sizes, 0),
                            prior=joint_phoneme_posteriors(probs, lens, ids.cuda(), sizes, 0, 0.05)))

    def want_line(k, x, which):
        s = per_set[k]
        canonical = " ".join(i2c[i] for i in s["ids"][x][:s["sizes"][x]])
        post = s[which][x]
        assert post is not None and len(post[0]) == s["sizes"][x] and len(post[1]) == s["sizes"][x] + 1
        return posterior_line(diagnose_posterior(s["decoded"][x], canonical, post[0], beam, vocab.index2word), "jpost  : ")

    for x, u in enumerate(utts):
        assert after[u][:12] == before[u][:12] and len(after[u]) == 13, u          # one line behind 'score  :', nothing else
        assert after[u][12] == want_line(0, x, "uniform"), u
        assert "[-]" not in after[u][12]

    # --error_prior: other numbers on the same line, nothing else
    prior = _blocks(_run_infer(tmp_path, ["--joint_posteriors", "--error_prior", "0.05"]))
    changed = 0
    for x, u in enumerate(utts):
        assert prior[u][:12] == before[u][:12] and len(prior[u]) == 13 and prior[u][12] == want_line(0, x, "prior"), u
        changed += prior[u][12] != after[u][12]
    assert changed >= 1

    # with every other line: behind post, in front of nbest and pron, and the chosen candidate's
    rest = ["--timestamps", "--posteriors", "--pronunciations", "--nbest", "2"]
    base_t, with_t = _blocks(_run_infer(tmp_path, rest)), _blocks(_run_infer(tmp_path, rest + ["--joint_posteriors"]))
    moved = 0
    for x, u in enumerate(utts):
        assert [line for line in with_t[u] if not line.startswith("jpost  : ")] == base_t[u], u
        assert [line[:9] for line in with_t[u][12:]] == ["time   : ", "gop    : ", "post   : ", "jpost  : ", "nbest  : ", "nbest  : ", "pron   : "], u
        n = cand["counts"][x]
        ll = [per_set[k]["base"][x] for k in range(n)]
        chosen = max(range(n), key=lambda k: (ll[k], -k))
        assert with_t[u][15] == want_line(chosen, x, "uniform"), (u, chosen)
        assert [t.split("[")[0] for t in with_t[u][15][9:].split("] ")] == [t.split("[")[0] for t in with_t[u][14][9:].split("] ")], u
        moved += chosen != 0
    assert moved >= 1, "no utterance chose a later pronunciation: the candidate's own line went unchecked"
