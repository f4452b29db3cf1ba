"""mdd_ctc_nbest (csrc/ctc_nbest.hip) on the GPU: all ranks of an N-best list rescored in one launch.

The route it replaces is the yardstick for the bits: ``(-loglik).float()`` equals, bit for bit (NaN and the infinities included),
``hip_model.ctc_loss(lp, ids[n, :, :max_len], lens, nids[n], want_grad=False)`` for every rank n -- at every N that gives the launch
another shape (a partial last group, a wave without a rank, a wave with several; the counts come from csrc/plan.h through
tests/ctc_nbest_cases.plan), where the scan changes its labels per lane, at the LDS bound, for every class count and blank position, on
the edge rows, and with bad labels.  The float64 yardstick (CPU torch.nn.functional.ctc_loss on a double tensor) holds the values to the
bound tests/test_nbest.py holds the loop to, 1e-6 relative.  Then the memory discipline of the call, and BeamDecoder's chain on top."""
import os

import numpy as np
import pytest
import torch

from tests import ctc_nbest_cases as cc
from tests import mbr_reference as mr
from tests.helpers import GOLD, record_margin

pytestmark = pytest.mark.gpu
_WORST = [0.0]
SENT = -12345.678      # no log-likelihood of a case


def _dev(case, N=None):
    N = case.ids.shape[0] if N is None else N
    return (torch.from_numpy(np.array(case.lp)).cuda(), torch.from_numpy(np.array(case.lens)).cuda(),
            torch.from_numpy(np.array(case.ids[:N])).cuda(), torch.from_numpy(np.array(case.nids[:N])).cuda())


def _loop(lp, lens, ids, nids, blank, max_len):
    """The route the entry replaces: one ctc_loss call without gradient per rank; nll [N, B] fp32."""
    from ctc_attention_mispronunciation_amd import hip_model
    return torch.stack([hip_model.ctc_loss(lp, ids[n, :, :max_len], lens, nids[n], blank=blank, want_grad=False)[0] for n in range(ids.shape[0])])


_LOOPS = {}


def _case_loop(case, N):
    """The loop's nll of a case's first N ranks, computed once for the largest N asked and shared."""
    if case.name not in _LOOPS or _LOOPS[case.name].shape[0] < N:
        lp, lens, ids, nids = _dev(case, N)
        _LOOPS[case.name] = _loop(lp, lens, ids, nids, case.blank, case.max_len)
    return _LOOPS[case.name][:N]


def _nbest(case, N, **kw):
    from ctc_attention_mispronunciation_amd import hip_model
    lp, lens, ids, nids = _dev(case, N)
    ll = hip_model.ctc_nbest(lp, lens, ids, nids, blank=case.blank, max_len=case.max_len, **kw)
    assert ll.dtype == torch.float64 and ll.is_cuda and tuple(ll.shape) == (N, case.lp.shape[1])
    return ll


def _bits(ll):
    """(-loglik).float() as int32 words."""
    return (-ll).float().view(torch.int32)


def _assert_bits(ll, nll, tag):
    same = _bits(ll) == nll.view(torch.int32)
    assert bool(same.all()), (tag, (~same).nonzero()[:8].tolist(), ll[~same][:8].tolist(), nll[~same][:8].tolist())


def _yardstick(case, ll, N):
    ref = cc.reference(case.name, N)
    assert np.isfinite(ref).mean() >= 0.5, case.name
    worst = cc.loglik_rel_err(ll.cpu().numpy(), ref)
    print("%s N %d: worst |loglik - f64| / |f64| = %.3e (bound %.0e)" % (case.name, N, worst, cc.LOGLIK_RTOL))
    _WORST[0] = max(_WORST[0], worst)
    record_margin("ctc_nbest_loglik_rel", _WORST[0], cc.LOGLIK_RTOL)
    assert worst <= cc.LOGLIK_RTOL, (case.name, worst)


# ------------------------------------------------------------------------------------------- bit-equality with the loop
@pytest.mark.parametrize("kind,B", [("peaky", 3), ("dense", 3), ("dense", 6)])
def test_bits_are_the_loops_at_every_group_shape(kind, B):
    """N around the plan's waves and ranks per workgroup (csrc/plan.h, not guessed): a partial last group, waves without a rank, waves
    with several.  B = 3 keeps every N on the rule's first branch, B = 6 puts the long lists on its second."""
    case = cc.ragged(kind, B=B)
    p = cc.plan(40, B, 45, cc.MAX_N, case.max_len)
    w, h = p.waves, p.hyps_per_block
    assert p.fits and h == (4 if B == 3 else 10), p
    Ns = sorted(n for n in {1, 2, w - 1, w, w + 1, h - 1, h, h + 1, 2 * h + 3, 200, 256} if 1 <= n <= cc.MAX_N)
    nll = _case_loop(case, cc.MAX_N)
    for N in Ns:
        _assert_bits(_nbest(case, N), nll[:N], (kind, B, N))
    _yardstick(case, _nbest(case, 2 * h + 3), 2 * h + 3)


@pytest.mark.parametrize("waves,hpb", [(None, 1), (None, 3), (None, 8), (None, 64), (None, 256), (1, None), (4, 6), (16, None), (16, 40)])
def test_waves_and_ranks_per_workgroup_do_not_change_the_bits(waves, hpb, monkeypatch):
    """The sweep's switches (csrc/plan.h): any waves per workgroup, any ranks per workgroup, the same results."""
    case = cc.ragged("dense", B=6)
    for var in ("MDD_CTC_NBEST_WAVES", "MDD_CTC_NBEST_HPB"):
        monkeypatch.delenv(var, raising=False)
    want = _nbest(case, 200).view(torch.int64)
    if waves is not None:
        monkeypatch.setenv("MDD_CTC_NBEST_WAVES", str(waves))
    if hpb is not None:
        monkeypatch.setenv("MDD_CTC_NBEST_HPB", str(hpb))
    assert torch.equal(_nbest(case, 200).view(torch.int64), want)
    _assert_bits(_nbest(case, 35), _case_loop(case, cc.MAX_N)[:35], (waves, hpb))


@pytest.mark.parametrize("longest", [63, 64, 127, 128, 255])
def test_where_the_scan_changes_form(longest):
    case = cc.form(longest)
    assert cc.plan(300, 2, 45, 3, longest).NL == (1 if longest <= 63 else 2 if longest <= 127 else 4) and int(case.nids[0, 0]) == longest
    ll = _nbest(case, 3)
    _assert_bits(ll, _case_loop(case, 3), longest)
    _yardstick(case, ll, 3)


@pytest.mark.parametrize("Cn", [45, 256])
def test_the_lds_bound_itself(Cn):
    from ctc_attention_mispronunciation_amd import _lib, hip_model
    T = 1
    while hip_model.ctc_nbest_fits(T + 1, Cn, 14):
        T += 1
    assert T == 116 * 1024 // (4 * Cn)
    N = cc.plan(T, 1, Cn, cc.MAX_N, 14).hyps_per_block + 1
    case = cc.bound(Cn, T, N)
    ll = _nbest(case, N)
    _assert_bits(ll, _case_loop(case, N), (Cn, T))
    assert torch.isfinite(ll).all()
    lp = torch.zeros((T + 1, 1, Cn), device="cuda")
    with pytest.raises(_lib.MddError, match="mdd_ctc_nbest.*LDS"):
        hip_model.ctc_nbest(lp, [T + 1], torch.from_numpy(np.array(case.ids)).cuda(), torch.from_numpy(np.array(case.nids)).cuda(), max_len=14)


@pytest.mark.parametrize("Cn,blank", [(2, 0), (2, 1), (45, 0), (45, 22), (45, 44), (256, 0), (256, 100), (256, 255)])
def test_classes_and_blank_positions(Cn, blank):
    case = cc.ragged("dense", C=Cn, blank=blank)
    N = cc.plan(40, 3, Cn, cc.MAX_N, case.max_len).hyps_per_block + 15
    ll = _nbest(case, N)
    _assert_bits(ll, _case_loop(case, N), (Cn, blank))
    _yardstick(case, ll, N)


def test_peaky_rows_with_the_blank_at_the_last_class():
    case = cc.ragged("peaky", blank=44)
    ll = _nbest(case, 35)
    _assert_bits(ll, _case_loop(case, 35), "peaky blank 44")
    _yardstick(case, ll, 35)


# -------------------------------------------------------------------------------------------------------------------- rows
def test_edge_rows():
    """len = 0 with nids = 0 (0) and with nids > 0 (-inf); len < T; nids = 0 (the sum of the blank column); nids > max_len (clamped)."""
    from ctc_attention_mispronunciation_amd import hip_model
    T, B, Cn, N, max_len = 40, 4, 45, 19, 10
    lp_h = cc.dense_logp(2800, T, B, Cn)
    ids_h, nids_h = cc.draw_lists(2801, N, B, Cn, 0, 5, 8, pitch=T, max_len=max_len)
    ids_h[:, :, max_len:] = 7                       # valid labels behind max_len: a clamped row must stop at max_len all the same
    lens_h = np.array([0, 0, 30, 40], dtype=np.int32)
    nids_h[:, 0] = 0
    nids_h[4, 3] = nids_h[18, 2] = 0
    nids_h[2, 2], nids_h[9, 3] = max_len + 5, T
    ids_h[2, 2, :max_len] = ids_h[9, 3, :max_len] = np.arange(1, max_len + 1)
    lp, lens, ids, nids = (torch.from_numpy(a).cuda() for a in (lp_h, lens_h, ids_h, nids_h))
    ll = hip_model.ctc_nbest(lp, lens, ids, nids, max_len=max_len)
    _assert_bits(ll, _loop(lp, lens, ids, nids, 0, max_len), "edge rows")
    ll = ll.cpu().numpy()
    assert (ll[:, 0] == 0.0).all() and (ll[:, 1] == -np.inf).all() and np.isfinite(ll[:, 2:]).all()
    for n, b in ((4, 3), (18, 2)):
        want = float(lp_h[:lens_h[b], b, 0].astype(np.float64).sum())
        assert abs(ll[n, b] - want) <= cc.LOGLIK_RTOL * abs(want), (n, b, ll[n, b], want)
    # the clamped rows score what the same ids score with nids = max_len
    nids2 = nids_h.copy()
    nids2[2, 2] = nids2[9, 3] = max_len
    ll2 = hip_model.ctc_nbest(lp, lens, ids, torch.from_numpy(nids2).cuda(), max_len=max_len).cpu().numpy()
    assert np.array_equal(ll, ll2)
    # max_len = 0: every hypothesis is the empty one
    ll0 = hip_model.ctc_nbest(lp, lens, ids, nids, max_len=0).cpu().numpy()
    assert np.array_equal(ll0, np.broadcast_to(np.array([0.0, 0.0, ll[18, 2], ll[4, 3]]), (N, B)))


def test_repeats_the_frames_cannot_hold_are_minus_infinity():
    """tests/test_nbest.py's hand-made slices: k k needs three frames and has two."""
    from ctc_attention_mispronunciation_amd import hip_model, synth
    logp = np.stack([synth.peaky_logp(6, 45, 1 + b, seed=1800 + b) for b in range(2)], axis=1)
    ids = np.zeros((3, 2, 6), dtype=np.int32)
    ids[0, :, :2] = (7, 7)
    ids[1, :, :2] = (7, 9)
    ids[2, :, :3] = (5, 5, 5)
    nids = np.array([[2, 2], [2, 2], [3, 3]], dtype=np.int32)
    lp, lens, ids_d, nids_d = torch.from_numpy(logp).cuda(), torch.tensor([2, 6], dtype=torch.int32).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(nids).cuda()
    ll = hip_model.ctc_nbest(lp, lens, ids_d, nids_d, max_len=3)
    _assert_bits(ll, _loop(lp, lens, ids_d, nids_d, 0, 3), "repeats")
    ll = ll.cpu().numpy()
    assert (ll[:, 0] == -np.inf).tolist() == [True, False, True] and np.isfinite(ll[:, 1]).all() and np.isfinite(ll[1, 0])


def test_a_bad_label_is_nan_for_its_own_row_alone():
    from ctc_attention_mispronunciation_amd import hip_model
    case = cc.ragged("dense")
    N = 19
    lp, lens, ids, nids = _dev(case, N)
    clean = hip_model.ctc_nbest(lp, lens, ids, nids, max_len=case.max_len)
    bad = ids.clone()
    rows = ((3, 1, 2, -1), (17, 2, 0, 45), (8, 0, int(case.nids[8, 0]) - 1, 1 << 30), (16, 1, 1, -(1 << 31)))
    for n, b, i, v in rows:
        assert i < case.nids[n, b]
        bad[n, b, i] = v
    got = hip_model.ctc_nbest(lp, lens, bad, nids, max_len=case.max_len)
    _assert_bits(got, _loop(lp, lens, bad, nids, 0, case.max_len), "bad labels")
    hit = torch.zeros((N, 3), dtype=torch.bool, device="cuda")
    for n, b, _, _ in rows:
        hit[n, b] = True
    assert bool(torch.isnan(got[hit]).all()) and not bool(torch.isnan(got[~hit]).any())
    assert torch.equal(got[~hit].view(torch.int64), clean[~hit].view(torch.int64))


# ------------------------------------------------------------------------------------------------------- memory discipline
def _raw(lp, lens, ids, nids, max_len, out, blank=0):
    from ctc_attention_mispronunciation_amd import _lib
    T, B, Cn = lp.shape
    N, _, pitch = ids.shape
    p = _lib.ptr
    _lib.check(_lib.lib().mdd_ctc_nbest(p(lp), T, B, Cn, p(lens), p(ids), pitch, p(nids), N, max_len, blank, p(out), _lib.current_stream_ptr()))


def test_memory_discipline():
    """Ids past nids are never read, frames past len neither; every element of loglik is written and nothing behind it; two calls and a
    call on a side stream give the same bits."""
    from ctc_attention_mispronunciation_amd import hip_model
    case = cc.ragged("dense")
    N, B, spare = 35, 3, 64
    lp, lens, ids, nids = _dev(case, N)
    want = hip_model.ctc_nbest(lp, lens, ids, nids, max_len=case.max_len)
    assert bool(torch.isfinite(want).all())
    out = torch.full((N * B + spare,), SENT, dtype=torch.float64, device="cuda")
    _raw(lp, lens, ids, nids, case.max_len, out)
    assert torch.equal(out[:N * B].view(torch.int64), want.reshape(-1).view(torch.int64)) and bool((out[N * B:] == SENT).all())
    poisoned = torch.from_numpy(mr.poisoned(5, np.array(case.ids[:N]), np.array(case.nids[:N]), 45)).cuda()
    assert not torch.equal(poisoned, ids)
    assert torch.equal(hip_model.ctc_nbest(lp, lens, poisoned, nids, max_len=case.max_len).view(torch.int64), want.view(torch.int64))
    holes = lp.clone()
    for b, n in enumerate(case.lens):
        holes[int(n):, b, :] = float("nan")
    assert bool(torch.isnan(holes).any())
    assert torch.equal(hip_model.ctc_nbest(holes, lens, ids, nids, max_len=case.max_len).view(torch.int64), want.view(torch.int64))
    assert torch.equal(hip_model.ctc_nbest(lp, lens, ids, nids, max_len=case.max_len).view(torch.int64), want.view(torch.int64))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        again = hip_model.ctc_nbest(lp, lens, ids, nids, max_len=case.max_len)
    side.synchronize()
    assert torch.equal(again.view(torch.int64), want.view(torch.int64))
    # int32 device tensors pass through with no copy; host arrays and other integer types are converted
    from_host = hip_model.ctc_nbest(lp, [int(v) for v in case.lens], np.array(case.ids[:N]).astype(np.int64), np.array(case.nids[:N]), max_len=case.max_len)
    assert torch.equal(from_host.view(torch.int64), want.view(torch.int64))


# ------------------------------------------------------------------------------------------------------------------- chain
def _decoder(beam):
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    return BeamDecoder(synth.phone_table_41(), beam_width=beam, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=0.2)


@pytest.mark.parametrize("beam", [10, 200])
def test_decoder_chain_gives_the_loops_bytes(beam, monkeypatch):
    """decode_nbest_ids -> nbest_loglik at beam 10 (mdd_beam_nbest) and beam 200, N = 200 (mdd_beam_wide): one ctc_nbest call, the array
    of the per-rank loop; decode_nbest and decode_mbr return what they return with the new entry switched off."""
    from ctc_attention_mispronunciation_amd import _lib, hip_model
    T, B, Cn = 40, 3, 45
    dec = _decoder(beam)
    lp = torch.from_numpy(cc.peaky_logp(1700, T, B, Cn)).cuda()
    lens = list(cc.RAGGED)
    assert bool(_lib.lib().mdd_beam_fits(T, B, Cn, beam)) == (beam == 10)
    ids, nids, status, _ = dec.decode_nbest_ids(lp, lens)
    assert ids.shape[0] == beam and not bool(status.any())
    longest = int(nids.max())
    calls = []
    real = hip_model.ctc_nbest
    monkeypatch.setattr(hip_model, "ctc_nbest", lambda *a, **k: calls.append(1) or real(*a, **k))
    ll = dec.nbest_loglik(lp, lens, ids, nids, max_len=longest)
    assert calls == [1] and ll.dtype == np.float64 and ll.shape == (beam, B)
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    loop = -_loop(lp, lens_d, ids, nids, 0, longest).double().cpu().numpy()
    assert np.array_equal(ll, loop, equal_nan=True) and np.array_equal(np.signbit(ll), np.signbit(loop)) and np.isfinite(ll).any()
    got_nbest, got_mbr = dec.decode_nbest(lp, lens, nbest=min(beam, 20)), dec.decode_mbr(lp, lens, nbest=min(beam, 20))
    n_new = len(calls)
    assert n_new == 3
    monkeypatch.setattr(hip_model, "ctc_nbest_fits", lambda *a: False)
    assert dec.decode_nbest(lp, lens, nbest=min(beam, 20)) == got_nbest and dec.decode_mbr(lp, lens, nbest=min(beam, 20)) == got_mbr
    assert len(calls) == n_new and np.array_equal(dec.nbest_loglik(lp, lens, ids, nids, max_len=longest), ll, equal_nan=True)
