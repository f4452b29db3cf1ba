"""Timed diagnosis: ``infer_core.diagnose_timed`` on hand-built spans (host), then ``decode_timed`` / ``infer(..., timestamps=True)``
over G13's batch on the GPU (the default output must stay G13's byte for byte; the two extra lines must be consistent with it)."""
import io
import math
import os
import re
import types

import pytest

from tests.helpers import GOLD, jload

SPF = 0.04
BASE_KEYS = ("decoded", "canonical", "path", "insertions", "substitutions", "deletions", "correct", "del_sub", "score", "printed")


def _decoder():
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import Decoder
    return Decoder({0: "blank"}, space_idx=-1, blank_index=0)


def _spans(n, base):
    """Span i = (base + 10 i, base + 10 i + 5, -(i + 1) / 8): the token index can be read back from any of the three numbers."""
    return [(base + 10 * i, base + 10 * i + 5, -(i + 1) / 8.0) for i in range(n)]


def _run(decoded, canonical, spans="auto", canon_spans="auto", to_display=None):
    from ctc_attention_mispronunciation_amd.infer_core import diagnose, diagnose_timed
    dec, can = decoded.split(), canonical.split()
    spans = _spans(len(dec), 0) if spans == "auto" else spans
    canon_spans = _spans(len(can), 1000) if canon_spans == "auto" else canon_spans
    d = diagnose_timed(decoded, spans, canonical, canon_spans, _decoder(), SPF, to_display)
    base = diagnose(decoded, canonical, _decoder(), to_display)
    assert {k: d[k] for k in BASE_KEYS} == base and set(d) == set(BASE_KEYS) | {"times", "gop"}
    assert len(d["times"]) == len(d["gop"]) == len(d["path"])
    # which decoded / canonical token every row got, read back from the spans
    dec_idx = [None if t is None else int(round(t[0] / SPF)) // 10 for t in d["times"]]
    can_idx = [None if g is None else int(round(-g * 8)) - 1 for g in d["gop"]]
    for row, op in enumerate(d["path"]):
        assert (dec_idx[row] is None) == (op == "D" or spans is None), (row, op)
        assert (can_idx[row] is None) == (op == "I" or canon_spans is None), (row, op)
        if dec_idx[row] is not None:
            i = dec_idx[row]
            assert dec[i].replace("err", "") == d["decoded"][row] or to_display is not None
            start, end, conf = d["times"][row]
            assert start == spans[i][0] * SPF and end == spans[i][1] * SPF and conf == math.exp(spans[i][2])
        if can_idx[row] is not None:
            assert can[can_idx[row]] == d["canonical"][row] or to_display is not None
            assert d["gop"][row] == canon_spans[can_idx[row]][2]
    return d, dec_idx, can_idx


def test_sil_at_both_ends_and_inside():
    d, di, ci = _run("sil a b sil c sil", "sil a b c sil")
    assert d["path"] == ["-", "-", "-"] and di == [1, 2, 4] and ci == [1, 2, 3]


def test_err_token_is_removed_with_its_span():
    d, di, ci = _run("a err b", "a b")
    assert d["path"] == ["-", "-"] and di == [0, 2] and ci == [0, 1]


def test_leading_insertions_and_repeated_first_phone():
    d, di, ci = _run("x y z a b", "a b")                 # three leading insertions: the last one is kept
    assert d["path"] == ["I", "-", "-"] and d["decoded"] == ["z", "a", "b"] and di == [2, 3, 4] and ci == [None, 0, 1]
    d, di, ci = _run("sil a a b c", "a b c")             # a leading insertion that repeats the first aligned phone is dropped
    assert d["path"] == ["-", "-", "-"] and d["decoded"] == ["a", "b", "c"] and ci == [0, 1, 2]
    assert di[1:] == [3, 4] and di[0] in (1, 2)
    d, di, ci = _run("q q a a b", "a b")                 # both rules at once
    assert d["decoded"][-2:] == ["a", "b"] and di[-2:] == [3, 4] and ci[-2:] == [0, 1]


def test_substitution_deletion_insertion_in_the_middle():
    d, di, ci = _run("a x c e f q g", "a b c d e f g")
    assert d["path"] == ["-", "S", "-", "D", "-", "-", "I", "-"]
    assert di == [0, 1, 2, None, 3, 4, 5, 6] and ci == [0, 1, 2, 3, 4, 5, None, 6]
    assert d["substitutions"] == ["b"] and d["deletions"] == ["d"] and d["insertions"] == ["q"]


def test_display_names_do_not_move_the_spans():
    d, di, ci = _run("a x c", "a b c", to_display={"A": "AA", "X": "XX", "B": "BB"})
    assert d["decoded"] == ["AA", "XX", "c"] and d["canonical"] == ["AA", "BB", "c"] and di == [0, 1, 2] and ci == [0, 1, 2]


def test_absent_alignments_give_none():
    d, di, ci = _run("a x c e", "a b c d e", canon_spans=None)
    assert d["gop"] == [None] * len(d["path"]) and any(t is not None for t in d["times"])
    d, di, ci = _run("a x c e", "a b c d e", spans=None)       # a beam winner without a feasible alignment
    assert d["times"] == [None] * len(d["path"]) and any(g is not None for g in d["gop"])


def test_count_mismatch_raises():
    from ctc_attention_mispronunciation_amd.infer_core import diagnose_timed
    with pytest.raises(ValueError, match="3 spans for 4 decoded"):
        diagnose_timed("a b sil c", _spans(3, 0), "a b c", _spans(3, 0), _decoder(), SPF)
    with pytest.raises(ValueError, match="4 spans for 3 canonical"):
        diagnose_timed("a b c", _spans(3, 0), "a b c", _spans(4, 0), _decoder(), SPF)


def test_timed_lines_format():
    from ctc_attention_mispronunciation_amd.infer_core import timed_lines
    d = dict(decoded=["a", "D", "q"], canonical=["a", "b", "I"], path=["-", "D", "I"],
             times=[(0.12, 0.2, 0.934), None, (0.2, 0.44, 0.5)], gop=[-0.071, -3.5, None])
    assert timed_lines(d) == ("time   : a[0.12-0.20 0.93] q[0.20-0.44 0.50]", "gop    : a[-0.07] b[-3.50]")
    d["times"], d["gop"] = [None] * 3, [None] * 3
    assert timed_lines(d) == ("time   : a[-] q[-]", "gop    : a[-] b[-]")


def test_seconds_per_frame_comes_from_the_loader():
    from ctc_attention_mispronunciation_amd.infer_core import seconds_per_frame
    assert seconds_per_frame(types.SimpleNamespace(n_skip_frame=2), 2) == pytest.approx(0.04, abs=1e-12)
    assert seconds_per_frame(types.SimpleNamespace(dataset=types.SimpleNamespace(n_skip_frame=3)), 2) == pytest.approx(0.06, abs=1e-12)
    with pytest.raises(ValueError):
        seconds_per_frame([], 2)


# ------------------------------------------------------------------------------------------------------------------- GPU
TIME_TOKEN = re.compile(r"^(\S+)\[(?:-|(\d+\.\d\d)-(\d+\.\d\d) (\d\.\d\d))\]$")


@pytest.mark.gpu
def test_infer_with_timestamps_over_g13(monkeypatch):
    import torch
    from tests.test_infer_batch import _case, _read_wav
    from ctc_attention_mispronunciation_amd import infer_core, synth
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    from ctc_attention_mispronunciation_amd.utils.data_loader import WavBatchLoader
    meta = jload("g13_infer.json")
    case = _case(meta, 64)
    geom = synth.Geometry(**synth.REFERENCE)
    hip = HipModel(geom, synth.synth_state_dict(geom, seed=11))
    model = lambda inputs, trans: hip.forward(inputs.to("cuda", torch.float32).contiguous(), trans.to("cuda", torch.int64).contiguous(),   # noqa: E731
                                              sync_errors=True)
    i2c = synth.phone_table_41()
    vocab = types.SimpleNamespace(index2word=i2c, word2index={v: k for k, v in i2c.items()})
    beam = BeamDecoder(i2c, beam_width=10, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=0.0)
    phonetic = types.SimpleNamespace(api_word_translation=lambda utterance: "")
    word_dict = {u: {"ipa": meta["utts"][u]["cmu"]} for u in meta["order"]}
    words = {u: meta["utts"][u]["word"] for u in meta["order"]}
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt")))
    loader = WavBatchLoader([(u, _read_wav(int(u)), meta["utts"][u]["canonical"]) for u in meta["order"]], vocab, 64, cmvn)

    def run(**kw):
        buf = io.StringIO()
        totals = infer_core.infer(phonetic, word_dict, loader, torch.device("cuda"), model, beam, vocab, words, False, out=buf, **kw)
        assert list(totals) == case["totals"]
        return buf.getvalue()

    assert run(timestamps=False) == case["stdout"]

    frames, results, spfs = [], [], []
    real_timed, real_decode = infer_core.diagnose_timed, beam.decode_timed

    def decode_timed(probs, lens):
        frames.extend(lens)
        return real_decode(probs, lens)

    def diagnose_timed(decoded, spans, canonical, canon_spans, decoder, spf, to_display=None):
        d = real_timed(decoded, spans, canonical, canon_spans, decoder, spf, to_display)
        results.append(d); spfs.append(spf)
        return d

    monkeypatch.setattr(beam, "decode_timed", decode_timed)
    monkeypatch.setattr(infer_core, "diagnose_timed", diagnose_timed)
    got = run(timestamps=True)
    lines = got.split("\n")
    assert "\n".join(l for l in lines if not l.startswith(("time   : ", "gop    : "))) == case["stdout"]
    assert len(results) == len(frames) == len(meta["order"]) and all(abs(s - 0.04) < 1e-12 for s in spfs)
    blocks = got.split("id     : ")[1:]
    assert len(blocks) == len(results)
    timed = 0
    for block, d, n in zip(blocks, results, frames):
        bl = block.split("\n")
        assert bl[11].startswith("score  : ") and bl[12].startswith("time   : ") and bl[13].startswith("gop    : ") and bl[14] == ""
        toks = [TIME_TOKEN.match(t) for t in re.findall(r"\S+\[[^\]]*\]", bl[12][9:])]
        assert all(toks) and [m.group(1) for m in toks] == [p for p in bl[6].split() if p != "D"]
        assert [m.group(1) for m in toks] == [p for p, op in zip(d["decoded"], d["path"]) if op != "D"]
        gtoks = re.findall(r"(\S+)\[([^\]]*)\]", bl[13][9:])
        assert [p for p, _ in gtoks] == [p for p in bl[4].split() if p != "I"]
        last = 0.0
        for t in d["times"]:
            if t is not None:
                start, end, conf = t
                assert last <= start < end <= n * 0.04 + 1e-9 and 0.0 < conf <= 1.0, (t, last, n)
                last = end
                timed += 1
        assert all(g is None or g <= 0.0 for g in d["gop"])
        assert all((t is None) == (op == "D") for t, op in zip(d["times"], d["path"])) or all(t is None for t in d["times"])
    assert timed > 0


@pytest.mark.gpu
def test_greedy_decode_timed_spans_are_the_argmax_runs():
    import numpy as np
    import torch
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import GreedyDecoder
    rs = np.random.default_rng(5)
    T, B, Cn = 60, 3, 45
    x = rs.standard_normal((T, B, Cn)) * 3.0
    lp = torch.log_softmax(torch.from_numpy(x), dim=-1).float()
    lens = [60, 41, 17]
    dec = GreedyDecoder(synth.phone_table_41(), space_idx=-1, blank_index=0)
    strings, spans = dec.decode_timed(lp, lens)
    assert strings == dec.decode(lp, lens)
    am = lp.numpy().argmax(axis=-1)
    for b in range(B):
        runs, t = [], 0
        while t < lens[b]:
            e = t
            while e < lens[b] and am[e, b] == am[t, b]:
                e += 1
            if am[t, b] != 0:
                runs.append((t, e, float(np.mean(lp.numpy()[t:e, b, am[t, b]].astype(np.float64)))))
            t = e
        assert [(s, e) for s, e, _ in spans[b]] == [(s, e) for s, e, _ in runs]
        assert np.allclose([m for _, _, m in spans[b]], [m for _, _, m in runs], rtol=0, atol=2e-5)   # fp32 sum of k <= 60 values in [-log 45, 0]: (k - 1) 2^-24 x 3.8
