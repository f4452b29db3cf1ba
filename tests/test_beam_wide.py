"""mdd_beam_wide (csrc/beam_wide.hip) on the GPU, and BeamDecoder / infer routed to it where mdd_beam and mdd_beam_nbest refuse on size.

The yardsticks are oracle.beam (winners, statuses, scores) and tests/nbest_reference.nbest (ranked lists), tied to the reference's own
BeamDecoder at beam 200 by G17; the cases and their robustness are tests/test_beam_wide_reference.py's.  A comparison asserts ids, nids
and status exactly, scores within SCORE_RTOL relative (the two sides round exp(logp) to fp32 with different libm's), NaN scores and no
ids on error rows, every output entry written, nothing written past a hypothesis or behind the arrays.  Where mdd_beam_nbest accepts the
shape too, the two entries must give the same bits."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch

from tests import nbest_reference as nr
from tests.helpers import GOLD, record_margin
from tests.test_beam_wide_reference import (BOTH_CASES, BY_NAME, ERROR_CASE, LONG_CASES, MANY_CASE, NBEST_CASE, TIE_CASES, WIDE_CASES, g17,
                                            g17_lists)
from tests.test_decoders import MDD_ERR_ARG, MDD_OK, SCORE_RTOL, SENT_F, SENT_I, SPARE, _L, _dev, _ptr, expected, gpu_beam, inputs
from tests.test_nbest import gpu_nbest

pytestmark = pytest.mark.gpu
_WORST = [0.0]


def gpu_wide(logp, lens, lm, beam, blank, alpha, nbest, workspace=None, workspace_bytes=0):
    """One mdd_beam_wide call on sentinel-filled outputs: (rc, ids [N,B,T], nids [N,B], status [B], score [N,B]) as numpy, with SPARE
    sentinel rows behind every array that must come back untouched (tests/test_nbest.py: gpu_nbest)."""
    T, B, Cn = logp.shape
    lens_dev = np.concatenate([np.asarray(lens, dtype=np.int32), np.full(SPARE, min(T, 2), dtype=np.int32)])
    d_lp, d_len, d_lm = _dev(logp), _dev(lens_dev), _dev(np.asarray(lm, dtype=np.float64))
    ids = torch.full((nbest * B + SPARE, T), SENT_I, dtype=torch.int32, device="cuda")
    nids = torch.full((nbest * B + SPARE,), SENT_I, dtype=torch.int32, device="cuda")
    st = torch.full((B + SPARE,), SENT_I, dtype=torch.int32, device="cuda")
    sc = torch.full((nbest * B + SPARE,), SENT_F, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = _L().mdd_beam_wide(_ptr(d_lp), T, B, Cn, _ptr(d_len), beam, blank, _ptr(d_lm), C.c_double(alpha), nbest, _ptr(ids), _ptr(nids),
                            _ptr(st), _ptr(sc), None if workspace is None else _ptr(workspace), C.c_int64(workspace_bytes), None)
    torch.cuda.synchronize()
    ids, nids, st, sc = ids.cpu().numpy(), nids.cpu().numpy(), st.cpu().numpy(), sc.cpu().numpy()
    n = nbest * B
    assert (ids[n:] == SENT_I).all() and (nids[n:] == SENT_I).all() and (st[B:] == SENT_I).all() and (sc[n:] == SENT_F).all(), \
        "rows past the outputs were written"
    return rc, ids[:n].reshape(nbest, B, T), nids[:n].reshape(nbest, B), st[:B], sc[:n].reshape(nbest, B)


def _check_layout(tag, ids, nids, st, sc):
    """What every call must leave: all of nids / status / score written, error rows with nothing but the status, descending scores,
    nothing written past a hypothesis."""
    assert (nids != SENT_I).all() and (st != SENT_I).all() and (sc != SENT_F).all(), ("an output entry was not written", tag)
    bad = st != 0
    assert (nids[:, bad] == 0).all() and np.isnan(sc[:, bad]).all() and (ids[:, bad] == SENT_I).all(), tag
    assert (nids[:, ~bad] >= 1).all() and np.isfinite(sc[:, ~bad]).all() and (np.diff(sc[:, ~bad], axis=0) <= 0).all(), tag
    for n in range(ids.shape[0]):
        for b in range(ids.shape[1]):
            assert (ids[n, b, nids[n, b]:] == SENT_I).all() and (ids[n, b, :nids[n, b]] != SENT_I).all(), (tag, n, b)


def _record(rel):
    _WORST[0] = max(_WORST[0], rel)
    record_margin("beam_wide_score_rel", _WORST[0], SCORE_RTOL)


def check_winner(case, rows=None, nbest=1):
    """The winner (slice 0), status and score against oracle.beam on `rows` (default: all)."""
    logp, lens, lm = inputs(case)
    want, wst, wsc = expected(case)
    rc, ids, nids, st, sc = gpu_wide(logp, lens, lm, case.beam, case.blank, case.alpha, nbest)
    assert rc == MDD_OK, _L().mdd_last_error().decode()
    _check_layout(case.name, ids, nids, st, sc)
    worst = 0.0
    for b in (range(case.B) if rows is None else rows):
        assert st[b] == wst[b], (case.name, b)
        assert ids[0, b, :nids[0, b]].tolist() == want[b], (case.name, b)
        if wst[b] == 0:
            worst = max(worst, abs(sc[0, b] - wsc[b]) / abs(wsc[b]))
    print("%s: max relative score difference %.3e" % (case.name, worst))
    _record(worst)
    assert worst <= SCORE_RTOL, (case.name, worst)
    return ids, nids, st, sc


def check_lists(case, nbest):
    """All `nbest` slices against the Python yardstick's ranked list."""
    logp, lens, lm = inputs(case)
    rows, lists = nr.case_lists(case, "torch")
    rc, ids, nids, st, sc = gpu_wide(logp, lens, lm, case.beam, case.blank, case.alpha, nbest)
    assert rc == MDD_OK, _L().mdd_last_error().decode()
    _check_layout(case.name, ids, nids, st, sc)
    worst = 0.0
    for (final, status), b in zip(lists, rows):
        assert status == st[b] == 0, (case.name, b)
        for n in range(nbest):
            want_ids, want_s = final[n]
            assert ids[n, b, :nids[n, b]].tolist() == want_ids, (case.name, b, n)
            worst = max(worst, abs(sc[n, b] - want_s) / abs(want_s))
    print("%s nbest %d: max relative score difference %.3e" % (case.name, nbest, worst))
    _record(worst)
    assert worst <= SCORE_RTOL, (case.name, worst)
    return sc


# ---------------------------------------------------------------------------------- 1. the drop-in decoder at its defaults (G17)
def _i2c():
    from ctc_attention_mispronunciation_amd import synth
    return synth.phone_table_41()


@pytest.mark.parametrize("kind", ["peaky", "flat"])
def test_default_constructor_decodes_like_the_reference(kind):
    """``BeamDecoder(int2char, lm_path=...)`` as a user copies it from the reference: beam_width 200, lm_alpha 0.01."""
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    meta, g = g17()
    i2c = _i2c()
    dec = BeamDecoder(i2c, lm_path=os.path.join(GOLD, "lm_synth45.arpa"))
    assert dec.beam_width == 200 and dec.lm_alpha == 0.01 and dec.blank_index == 0
    lp, lens = torch.from_numpy(g[kind]).cuda(), g["lens"].tolist()
    assert dec.decode(lp, lens) == meta["batches"][kind]["best"]["default"]
    ids, nids, st, sc = (t.cpu().numpy() for t in dec.decode_nbest_ids(lp, lens))
    assert ids.shape == (200, 4, 40) and (st == 0).all()
    for b in range(4):
        want_ids, want_s = g17_lists(g, "default", kind, b)
        assert [ids[n, b, :nids[n, b]].tolist() for n in range(200)] == want_ids, b
        np.testing.assert_allclose(sc[:, b], want_s, rtol=SCORE_RTOL, atol=0)
    dec100 = BeamDecoder(i2c, beam_width=100, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=0.25)
    assert dec100.decode(lp, lens) == meta["batches"][kind]["best"]["b100"]


# ------------------------------------------------------------------------------------ 2. / 3. shapes only the wide entry accepts
@pytest.mark.parametrize("name", [c.name for c in WIDE_CASES + LONG_CASES])
def test_wide_only_shapes_against_oracle(name):
    case = BY_NAME[name]
    _, _, st, _ = check_winner(case)
    if case in WIDE_CASES:
        assert st.tolist() == [0, 0, 0, 1]                 # the row of length 0: IndexError
    assert _L().mdd_beam_fits(case.T, case.B, case.C, case.beam) == 0


# ----------------------------------------------------------------------------------------------- 4. same bits as mdd_beam_nbest
@pytest.mark.parametrize("name", [c.name for c in BOTH_CASES])
def test_wide_gives_the_bits_of_mdd_beam_nbest(name, monkeypatch):
    for var in ("MDD_BEAM_GENERIC", "MDD_BEAM_W"):
        monkeypatch.delenv(var, raising=False)
    case = BY_NAME[name]
    logp, lens, lm = inputs(case)
    _, wst, _ = expected(case)
    assert _L().mdd_beam_fits(case.T, case.B, case.C, case.beam) == 1
    rc, ids0, nids0, st0, sc0 = gpu_nbest(logp, lens, lm, case.beam, case.blank, case.alpha, case.beam)
    assert rc == MDD_OK, _L().mdd_last_error().decode()
    rc, ids, nids, st, sc = gpu_wide(logp, lens, lm, case.beam, case.blank, case.alpha, case.beam)
    assert rc == MDD_OK, _L().mdd_last_error().decode()
    _check_layout(name, ids, nids, st, sc)
    np.testing.assert_array_equal(st, wst)
    assert (st == st0).all() and (nids == nids0).all() and (ids == ids0).all(), name
    assert (sc.view(np.int64) == sc0.view(np.int64)).all(), name
    rc, ids1, nids1, st1, sc1 = gpu_wide(logp, lens, lm, case.beam, case.blank, case.alpha, 1)
    assert rc == MDD_OK
    assert (st1 == st).all() and (nids1[0] == nids[0]).all() and (ids1[0] == ids[0]).all() and (sc1[0].view(np.int64) == sc[0].view(np.int64)).all()


# ------------------------------------------------------------------------------------------------- 5. ties past 64 beams
@pytest.mark.parametrize("name", [c.name for c in TIE_CASES])
def test_wide_ties_keep_the_order_of_the_final_beam(name):
    case = BY_NAME[name]
    sc = check_lists(case, case.beam)
    assert (np.diff(sc, axis=0) == 0).any(), "no exact tie inside a list"
    check_winner(case)


# ----------------------------------------------------------------------------------------------------- 6. the first error
def test_wide_first_error_in_the_reference_s_order():
    _, _, st, _ = check_winner(ERROR_CASE, nbest=3)
    assert set(st.tolist()) == {1, 2, 3}          # (no clean row at this width: tests/test_beam_wide_reference.py::test_error_rows_at_a_wide_beam)


# ------------------------------------------------------------------------------------------------------------ 7. N best
def test_wide_whole_list_at_the_default_width():
    assert NBEST_CASE.beam == 200
    check_lists(NBEST_CASE, 200)


# --------------------------------------------------------------------------------------------------------- 8. workspace
def test_wide_caller_workspace():
    case = BY_NAME["wide_flat_b200_C45_T40_a0.01_blank0"]
    logp, lens, lm = inputs(case)
    need = _L().mdd_beam_wide_workspace_bytes(case.T, case.B, case.C, case.beam)
    rc, ids0, nids0, st0, sc0 = gpu_wide(logp, lens, lm, case.beam, case.blank, case.alpha, 5)
    assert rc == MDD_OK, _L().mdd_last_error().decode()
    guard = 64
    ws = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    rc, ids, nids, st, sc = gpu_wide(logp, lens, lm, case.beam, case.blank, case.alpha, 5, ws, need)
    assert rc == MDD_OK, _L().mdd_last_error().decode()
    assert (ws[need:] == 0x5A).all(), "written behind the stated workspace"
    assert (st == st0).all() and (nids == nids0).all() and (ids == ids0).all() and (sc.view(np.int64) == sc0.view(np.int64)).all()
    ws.fill_(0x5A)
    rc, ids, nids, st, sc = gpu_wide(logp, lens, lm, case.beam, case.blank, case.alpha, 5, ws, need - 1)
    assert rc == MDD_ERR_ARG
    msg = _L().mdd_last_error().decode()
    assert msg.startswith("mdd_beam_wide") and "workspace" in msg, msg
    assert (ids == SENT_I).all() and (nids == SENT_I).all() and (st == SENT_I).all() and (sc == SENT_F).all()
    assert (ws == 0x5A).all()


# -------------------------------------------------------------------------------------------- 9. more utterances than CUs
def test_wide_more_utterances_than_compute_units():
    case = MANY_CASE
    assert case.B == 257
    rows = nr.spread_rows(case.B, case.port_rows)
    _, _, st, _ = check_winner(case, rows=rows)
    _, wst, _ = expected(case)
    np.testing.assert_array_equal(st, wst)


# ----------------------------------------------------------------------------------------------------------- 10. routing
def _decoder(beam, alpha=0.2):
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    return BeamDecoder(_i2c(), beam_width=beam, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=alpha)


@contextlib.contextmanager
def _count_wide_calls(monkeypatch):
    """The library's mdd_beam_wide wrapped to count its calls (the router's choice cannot be seen from the outputs: the bits agree)."""
    L, calls = _L(), []
    real = L.mdd_beam_wide

    def counting(*args):
        calls.append(args[1:6])
        return real(*args)
    monkeypatch.setattr(L, "mdd_beam_wide", counting)
    try:
        yield calls
    finally:
        monkeypatch.setattr(L, "mdd_beam_wide", real)


def test_decoder_routes_by_mdd_beam_fits(monkeypatch):
    for var in ("MDD_BEAM_GENERIC", "MDD_BEAM_W"):
        monkeypatch.delenv(var, raising=False)
    _, g = g17()
    logp, lens = g["peaky"], g["lens"].tolist()
    lp = torch.from_numpy(logp).cuda()
    with _count_wide_calls(monkeypatch) as calls:
        dec = _decoder(10)
        ids, nids, st, sc = (t.cpu().numpy() for t in dec.decode_ids(lp, lens))
        rc, ids0, nids0, st0, sc0 = gpu_beam(logp, lens, dec.lm.dense_table(_i2c(), 45), 10, 0, 0.2)
        assert rc == MDD_OK and calls == []
        assert (st == st0).all() and (nids == nids0).all() and (sc.view(np.int64) == sc0.view(np.int64)).all()
        for b in range(4):
            assert (ids[b, :nids[b]] == ids0[b, :nids0[b]]).all()
        assert tuple(dec.decode_nbest_ids(lp, lens)[0].shape) == (10, 4, 40) and calls == []
        wide = _decoder(200)
        strings = wide.decode(lp, lens)
        assert len(calls) == 1 and calls[0] == (40, 4, 45, calls[0][3], 200)
        timed, spans = wide.decode_timed(lp, lens)
        assert timed == strings and len(spans) == 4
        for s, span in zip(strings, spans):
            assert span is None or len(span) == len(s.split(" "))
        records = wide.decode_nbest(lp, lens, nbest=4)
        assert [r[0][0] for r in records] == strings and all(len(r) == 4 for r in records)
        for r in records:
            assert r[0][1] >= r[1][1] >= r[2][1] >= r[3][1] and all(np.isfinite(x[1]) for x in r)
            assert abs(sum(x[3] for x in r) - 1.0) < 1e-12
        ll = wide.nbest_loglik(lp, lens, *wide.decode_nbest_ids(lp, lens, 4)[:2])
        assert ll.shape == (4, 4) and [x[2] for x in records[0]] == ll[:, 0].tolist()
        long = _dev(inputs(BY_NAME["long_b64_C45_T664"])[0])                             # a long utterance at a beam mdd_beam takes
        n = len(calls)
        assert len(_decoder(64, 0.0).decode(long, [664])) == 1 and len(calls) == n + 1
    with pytest.raises(IndexError):
        _decoder(200).decode(lp, [40, 0, 40, 40])
    from ctc_attention_mispronunciation_amd._lib import MddError
    with pytest.raises(MddError, match="mdd_beam_wide"):
        _decoder(257).decode(lp, lens)


def test_infer_with_a_wide_beam(tmp_path, monkeypatch):
    """infer over tests/golden/vocabulary_single (tests/test_nbest_infer.py's set-up) with ``beam_width: 200`` and ``--nbest 3``: every block
    has three nbest lines, rank 1 carries the block's decoded phones.  With the shipped ``beam_width: 10`` the wide entry is never called
    and the output is the run's without the flag; a beam_width over 256 fails with the wide entry's message."""
    from ctc_attention_mispronunciation_amd._lib import MddError
    from tests.test_candidates import _blocks, _run_infer
    from tests.test_nbest_infer import LINE, _setup, _stable
    from ctc_attention_mispronunciation_amd import infer as infer_cli
    from ctc_attention_mispronunciation_amd.dict.phonetic_dict import Phonetic
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    from ctc_attention_mispronunciation_amd.utils.data_loader import Vocab, WavBatchLoader, frames_from_fraction
    monkeypatch.delenv("MDD_PRECISION", raising=False)
    model, i2c, arpa = _setup(tmp_path)
    conf = tmp_path / "conf.yaml"
    shipped = conf.read_text()
    assert "beam_width: 10\n" in shipped
    with _count_wide_calls(monkeypatch) as calls:
        plain = _run_infer(tmp_path, [])
        flagged = _run_infer(tmp_path, ["--nbest", "3"])
        assert calls == []
        assert [line for line in _stable(flagged, tmp_path) if not line.startswith("nbest  : ")] == _stable(plain, tmp_path)
        conf.write_text(shipped.replace("beam_width: 10\n", "beam_width: 200\n"))
        wide = _blocks(_run_infer(tmp_path, ["--nbest", "3"]))
        assert len(calls) >= 2 and all(c[4] == 200 for c in calls)
    assert sorted(wide) == sorted(_blocks(plain)) and len(wide) == 18
    # the decoder on the same posteriors: the batch WavBatchLoader forms, one plain forward (tests/test_nbest_infer.py)
    with contextlib.redirect_stdout(io.StringIO()):
        vocab = Vocab(str(tmp_path / "units"))
        items, _, _, _ = infer_cli.collect(str(tmp_path / "words"), Phonetic(os.path.join(GOLD, "cmudict_subset.dict")), False)
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt")))
    (inputs_, input_sizes, _, _, trans, _, utts, *_), = list(WavBatchLoader(items, vocab, 64, cmvn=cmvn))
    probs = model(inputs_, trans.cuda())
    lens = frames_from_fraction(input_sizes, probs.size(0)).numpy().tolist()
    strings = BeamDecoder(i2c, beam_width=200, blank_index=0, space_idx=-1, lm_path=arpa, lm_alpha=0.0).decode(probs, lens)
    for x, u in enumerate(utts):
        block = wide[u]
        got = [LINE.match(line) for line in block[12:]]
        assert len(block) == 15 and all(got), (u, block[12:])
        got = [m.groups() for m in got]
        assert [g_[0] for g_ in got] == ["1", "2", "3"] and [g_[1] for g_ in got] == ["*", " ", " "]
        assert float(got[0][3]) >= float(got[1][3]) >= float(got[2][3])
        assert got[0][2] == strings[x], u                                                # rank 1: the block's decoded phones
        assert ("Comp.  : %s/%s" % got[0][6:8]) == block[10], u                          # rank 1's Comp. is the block's own
    conf.write_text(shipped.replace("beam_width: 10\n", "beam_width: 257\n"))
    with pytest.raises(MddError, match="mdd_beam_wide"), contextlib.redirect_stdout(io.StringIO()):
        _run_infer(tmp_path, [])
