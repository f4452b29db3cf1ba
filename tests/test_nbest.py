"""mdd_beam_nbest on every kernel path of csrc/beam*.hip, BeamDecoder.decode_nbest on top of it (GPU).

Every (case, route) of tests/test_decoders.py runs at nbest = beam, 1 and min(3, beam) on sentinel-filled outputs.  Asserted: the
status is the oracle's; slice 0 (ids, nids, score) and the status are bit-identical to an mdd_beam call on the same inputs, for every
row; the ranked ids of all slices equal the yardstick's (tests/nbest_reference.py, pinned to the reference's own final sort by G16) on
the rows the case allows -- spread over the batch so that every wave position of a packed workgroup is hit -- with scores within
SCORE_RTOL relative; error rows have nids 0 and NaN in every slice; nothing is written past a row's nids, nor behind the arrays.
The cases are robust by tests/test_nbest_reference.py: the ranking does not hang on one ulp of exp(), and neighbouring scores are equal
or further apart than the two sides may differ."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import nbest_reference as nr
from tests.helpers import GOLD, record_margin
from tests.test_decoders import (MDD_ERR_ARG, MDD_OK, SCORE_RTOL, SENT_F, SENT_I, SPARE, _L, _dev, _log_softmax, _ptr, expected,
                                 fast_eligible, gpu_beam, inputs)
from tests.test_nbest_reference import LIMIT_CASES, NBEST_BY_NAME, NBEST_CASES

pytestmark = pytest.mark.gpu
_WORST = {}


def gpu_nbest(logp, lens, lm, beam, blank, alpha, nbest):
    """One mdd_beam_nbest call on sentinel-filled outputs: (rc, ids [N,B,T], nids [N,B], status [B], score [N,B]) as numpy.
    The outputs are hypothesis-major with pitch B, so the SPARE rows sit behind the last slice (ids, nids, score) and behind row B - 1
    (len, status): a wave of the last workgroup with b >= B that ran on would leave its status there, and its last slice behind the
    arrays' used part."""
    T, B, Cn = logp.shape
    lens_dev = np.concatenate([np.asarray(lens, dtype=np.int32), np.full(SPARE, min(T, 2), dtype=np.int32)])
    d_lp, d_len, d_lm = _dev(logp), _dev(lens_dev), _dev(np.asarray(lm, dtype=np.float64))
    ids = torch.full((nbest * B + SPARE, T), SENT_I, dtype=torch.int32, device="cuda")
    nids = torch.full((nbest * B + SPARE,), SENT_I, dtype=torch.int32, device="cuda")
    st = torch.full((B + SPARE,), SENT_I, dtype=torch.int32, device="cuda")
    sc = torch.full((nbest * B + SPARE,), SENT_F, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = _L().mdd_beam_nbest(_ptr(d_lp), T, B, Cn, _ptr(d_len), beam, blank, _ptr(d_lm), C.c_double(alpha), nbest, _ptr(ids), _ptr(nids),
                             _ptr(st), _ptr(sc), None)
    torch.cuda.synchronize()
    ids, nids, st, sc = ids.cpu().numpy(), nids.cpu().numpy(), st.cpu().numpy(), sc.cpu().numpy()
    n = nbest * B
    assert (ids[n:] == SENT_I).all() and (nids[n:] == SENT_I).all() and (st[B:] == SENT_I).all() and (sc[n:] == SENT_F).all(), \
        "rows past the outputs were written: a wave with b >= B did not return"
    return rc, ids[:n].reshape(nbest, B, T), nids[:n].reshape(nbest, B), st[:B], sc[:n].reshape(nbest, B)


def _set_route(route, monkeypatch):
    for var in ("MDD_BEAM_GENERIC", "MDD_BEAM_W"):
        monkeypatch.delenv(var, raising=False)
    if route == "generic":
        monkeypatch.setenv("MDD_BEAM_GENERIC", "1")
    elif route in ("w2", "w3"):
        monkeypatch.setenv("MDD_BEAM_W", route[1])
    elif route != "auto":
        raise AssertionError(route)


def check_nbest(case, route, monkeypatch):
    _set_route(route, monkeypatch)
    logp, lens, lm = inputs(case)
    _, wst, _ = expected(case)
    rows, lists = nr.case_lists(case, "torch")
    rc, ids1, nids1, st1, sc1 = gpu_beam(logp, lens, lm, case.beam, case.blank, case.alpha)
    assert rc == MDD_OK, _L().mdd_last_error().decode()
    kernel = "generic" if route == "generic" or not fast_eligible(case.beam, case.C) else ("fast_packed" if case.B > 64 else "fast")
    bad = wst != 0
    for N in sorted({case.beam, 1, min(3, case.beam)}, reverse=True):
        tag = (case.name, route, N)
        rc, ids, nids, st, sc = gpu_nbest(logp, lens, lm, case.beam, case.blank, case.alpha, N)
        assert rc == MDD_OK, _L().mdd_last_error().decode()
        assert (nids != SENT_I).all() and (st != SENT_I).all() and (sc != SENT_F).all(), ("an output entry was not written", tag)
        np.testing.assert_array_equal(st, wst, err_msg=str(tag))
        # slice 0 and the status: mdd_beam's outputs, bit for bit (the whole rows: what mdd_beam leaves untouched stays untouched here)
        assert (st == st1).all() and (nids[0] == nids1).all() and (ids[0] == ids1).all(), tag
        assert (sc[0].view(np.int64) == sc1.view(np.int64)).all(), tag
        # error rows: nothing but the status
        assert (nids[:, bad] == 0).all() and np.isnan(sc[:, bad]).all() and (ids[:, bad] == SENT_I).all(), tag
        assert (nids[:, ~bad] >= 1).all() and np.isfinite(sc[:, ~bad]).all() and (np.diff(sc[:, ~bad], axis=0) <= 0).all(), tag
        for n in range(N):
            for b in range(case.B):
                assert (ids[n, b, nids[n, b]:] == SENT_I).all(), (tag, n, b)       # nothing written past a hypothesis
                assert (ids[n, b, :nids[n, b]] != SENT_I).all(), (tag, n, b)
        # the yardstick's ranked list
        worst = 0.0
        for (final, status), b in zip(lists, rows):
            assert status == st[b], (tag, b)
            for n in range(N if status == 0 else 0):
                want_ids, want_s = final[n]
                assert ids[n, b, :nids[n, b]].tolist() == want_ids, (tag, b, n)
                worst = max(worst, abs(sc[n, b] - want_s) / abs(want_s))
        print("%s [%s -> %s] nbest %d: max relative score difference %.3e" % (case.name, route, kernel, N, worst))
        _WORST[kernel] = max(_WORST.get(kernel, 0.0), worst)
        record_margin("nbest_%s_score_rel" % kernel, _WORST[kernel], SCORE_RTOL)
        assert worst <= SCORE_RTOL, (tag, worst)


@pytest.mark.parametrize("name,route", [(c.name, r) for c in NBEST_CASES for r in c.routes])
def test_nbest_paths_against_yardstick(name, route, monkeypatch):
    check_nbest(NBEST_BY_NAME[name], route, monkeypatch)


@pytest.mark.parametrize("beam,Cn", sorted(LIMIT_CASES))
def test_nbest_T_limit(beam, Cn, monkeypatch):
    """The longest utterance mdd_beam accepts decodes at nbest = beam: the ending needs no LDS of its own.  One frame more is refused
    with MDD_ERR_ARG before any output is touched."""
    case = LIMIT_CASES[(beam, Cn)]
    check_nbest(case, "auto", monkeypatch)
    T = case.T + 1
    rs = np.random.Generator(np.random.PCG64(3))
    logp = _log_softmax(rs.standard_normal((T, 1, Cn)))
    lm = np.log(rs.uniform(0.01, 1.0, size=(Cn + 1, Cn + 1)))
    rc, ids, nids, st, sc = gpu_nbest(logp, [T], lm, beam, 0, 0.0, beam)
    assert rc == MDD_ERR_ARG
    msg = _L().mdd_last_error().decode()
    assert msg.startswith("mdd_beam_nbest") and "LDS" in msg, msg
    assert (ids == SENT_I).all() and (nids == SENT_I).all() and (st == SENT_I).all() and (sc == SENT_F).all()


# ------------------------------------------------------------------------------------------------ BeamDecoder.decode_nbest
def _decoder(beam=10, alpha=0.2):
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    i2c = synth.phone_table_41()
    return BeamDecoder(i2c, beam_width=beam, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=alpha), i2c


def _peaky(T=40, B=5, Cn=45, seed=1700):
    from ctc_attention_mispronunciation_amd import synth
    return np.stack([synth.peaky_logp(T, Cn, max(1, T // 8) + b, seed=seed + b) for b in range(B)], axis=1)


def test_decode_nbest_against_yardstick_and_ctc_oracle():
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import nbest_posteriors
    T, B, Cn, N = 40, 5, 45, 5
    dec, i2c = _decoder()
    logp = _peaky(T, B, Cn)
    lens = [40, 33, 40, 21, 37]
    table = dec.lm.dense_table(i2c, Cn)
    want = nr.nbest(logp, lens, table, 10, dec.lm_alpha, 0, "torch")
    want64 = nr.nbest(logp, lens, table, 10, dec.lm_alpha, 0, "f64")
    lp = torch.from_numpy(logp).cuda()
    got = dec.decode_nbest(lp, lens, nbest=N)
    assert [r[0][0] for r in got] == dec.decode(lp, lens)                  # record 0 is decode's string
    ids_d, nids_d, st_d, sc_d = dec.decode_nbest_ids(lp, lens, N)
    assert ids_d.is_cuda and tuple(ids_d.shape) == (N, B, T) and tuple(nids_d.shape) == (N, B) and tuple(sc_d.shape) == (N, B)
    assert tuple(dec.decode_nbest_ids(lp, lens)[0].shape) == (dec.beam_width, B, T)      # nbest defaults to beam_width
    worst_ll = 0.0
    for b in range(B):
        (final, status), (final64, _) = want[b], want64[b]
        assert status == 0 and len(got[b]) == N
        assert [ids for ids, _ in final[:N]] == [ids for ids, _ in final64[:N]], "the case ranks differently under the two exp flavours"
        ll_ref = []
        for n, (string, score, loglik, share) in enumerate(got[b]):
            want_ids, want_s = final[n]
            assert string == " ".join(i2c[k] for k in want_ids), (b, n)
            assert abs(score - want_s) <= SCORE_RTOL * abs(want_s), (b, n, score, want_s)
            nll, _ = oracle.ctc_loss(logp[:, b:b + 1], np.array([want_ids]), [lens[b]], [len(want_ids)], blank=0, want_grad=False)
            ref = -float(np.float64(nll[0]))
            ll_ref.append(ref)
            if np.isinf(ref):                    # the beam's hypothesis is no CTC path of these frames
                assert loglik == -np.inf and share == 0.0, (b, n)
            else:
                assert abs(loglik - ref) <= 1e-6 * abs(ref), (b, n, loglik, ref)
                worst_ll = max(worst_ll, abs(loglik - ref) / abs(ref))
        # a softmax moves by at most the largest shift of its inputs (d p_n = p_n (dx_n - sum_j p_j dx_j), so |d p_n| <= 2 p_n (1 - p_n)
        # max|dx| <= max|dx| / 2), and the inputs are within 1e-6 |loglik_n| of the oracle's
        ref_share = nbest_posteriors(ll_ref)
        bound = max(1e-6 * abs(v) for v in ll_ref if np.isfinite(v))
        for n, (_, _, _, share) in enumerate(got[b]):
            assert abs(share - ref_share[n]) <= bound, (b, n, share, ref_share[n])
        assert abs(sum(r[3] for r in got[b]) - 1.0) < 1e-12
    record_margin("nbest_rescore_loglik_rel", worst_ll, 1e-6)
    plain = dec.decode_nbest(lp, lens, nbest=N, rescore=False)
    assert [[(r[0], r[1]) for r in u] for u in plain] == [[(r[0], r[1]) for r in u] for u in got]
    assert all(r[2] is None and r[3] is None for u in plain for r in u)


def test_rescoring_gives_minus_infinity_to_what_is_no_ctc_path():
    """decode_nbest's rescoring (nbest_loglik) on hand-made slices: k k needs three frames and has two, so the oracle's nll is +inf;
    that hypothesis gets -inf and share 0, and a list of nothing else has no shares at all."""
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import nbest_posteriors
    dec, _ = _decoder()
    logp = _peaky(T=6, B=2, seed=1800)
    lens = [2, 6]
    ids = np.zeros((3, 2, 6), dtype=np.int32)
    ids[0, :, :2] = (7, 7)                       # infeasible in 2 frames, feasible in 6
    ids[1, :, :2] = (7, 9)
    ids[2, :, :3] = (5, 5, 5)                    # infeasible in 2 frames, feasible in 6 only just (5 frames)
    nids = np.array([[2, 2], [2, 2], [3, 3]], dtype=np.int32)
    ll = dec.nbest_loglik(torch.from_numpy(logp).cuda(), lens, torch.from_numpy(ids).cuda(), torch.from_numpy(nids).cuda(), max_len=3)
    assert ll.dtype == np.float64 and ll.shape == (3, 2)
    for n in range(3):
        nll, _ = oracle.ctc_loss(logp, ids[n].astype(np.int64), lens, nids[n], blank=0, want_grad=False)
        for b in range(2):
            if np.isinf(nll[b]):
                assert ll[n, b] == -np.inf, (n, b)
            else:
                assert abs(ll[n, b] + float(nll[b])) <= 1e-6 * abs(float(nll[b])), (n, b)
    assert np.isinf(ll[:, 0]).tolist() == [True, False, True] and np.isfinite(ll[:, 1]).all()
    share = nbest_posteriors(ll[:, 0])
    assert share.tolist() == [0.0, 1.0, 0.0]
    assert nbest_posteriors(ll[[0, 2], 0]) is None


def test_decode_nbest_raises_what_decode_raises():
    dec, _ = _decoder()
    lp = torch.from_numpy(_peaky()).cuda()
    for lens, exc in (([40, 0, 40, 40, 40], IndexError),):
        with pytest.raises(exc):
            dec.decode(lp, lens)
        with pytest.raises(exc):
            dec.decode_nbest(lp, lens, nbest=3)
        with pytest.raises(exc):
            dec.decode_nbest(lp, lens, nbest=3, rescore=False)
    bad = lp.clone()
    bad[5, 2, 9] = -120.0                         # exp(-120) == 0 in fp32: the reference's math.log raises ValueError
    with pytest.raises(ValueError):
        dec.decode(bad, [40] * 5)
    with pytest.raises(ValueError):
        dec.decode_nbest(bad, [40] * 5, nbest=3)
    with pytest.raises(ValueError, match="nbest must be"):
        dec.decode_nbest_ids(lp, [40] * 5, nbest=11)
