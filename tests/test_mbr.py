"""mdd_nbest_mbr on the GPU against the yardstick (tests/mbr_reference.py), and BeamDecoder.decode_mbr on top of it.

Every case calls the entry on sentinel-filled outputs.  `dist` and `ref_dist` must equal the yardstick everywhere; with weights k / 2^10
(every product and every sum exact in fp64, whatever the order) so must `risk`, `ref_risk` and `best`, bit for bit.  The shapes are the
smallest at which the kernel's forms change: N at the lane-block boundary (63, 64, 65) and at the limit, max_len at every word boundary
of the five instantiations (64 / 65, 128 / 129, 256 / 257, 512 / 513) and at the limit, with rows of exactly max_len, 0 and 1 ids next to
the others, C = 2, 45 and 256 with id 255 present, B = 1, 3 and 70.  With softmax weights the bound is the first-order bound of a sum of
N non-negative fp64 terms in any order, N 2^-52 sum_m w_m d(n, m), computed per entry from the yardstick."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import mbr_reference as mr
from tests.helpers import GOLD

pytestmark = pytest.mark.gpu
SENT_I, SENT_F = -77, -1234.5


def _L():
    from ctc_attention_mispronunciation_amd import _lib
    return _lib.lib()


def _dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a)).cuda()      # a copy: the shared inputs are read-only


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def gpu_mbr(ids, nids, status, weights, Cn, max_len, ref=None, ref_len=None, want_dist=True, want_ref_dist=True, want_ref_risk=True,
            own_workspace=False):
    """One mdd_nbest_mbr call on sentinel-filled outputs; the outputs as numpy arrays (None where not asked for).  ``own_workspace``: a
    caller workspace of exactly mdd_nbest_mbr_workspace_bytes, with a sentinel tail behind it that must come back untouched."""
    N, B, pitch = ids.shape
    has_ref = ref is not None
    d_ids, d_nids, d_st, d_w, d_ref, d_rl = _dev(ids), _dev(nids), _dev(status), _dev(np.asarray(weights, dtype=np.float64)), _dev(ref), _dev(ref_len)
    best = torch.full((B,), SENT_I, dtype=torch.int32, device="cuda")
    flag = torch.full((B,), SENT_I, dtype=torch.int32, device="cuda")
    risk = torch.full((N, B), SENT_F, dtype=torch.float64, device="cuda")
    dist = torch.full((B, N, N), SENT_I, dtype=torch.int32, device="cuda") if want_dist else None
    ref_dist = torch.full((N, B), SENT_I, dtype=torch.int32, device="cuda") if has_ref and want_ref_dist else None
    ref_risk = torch.full((B,), SENT_F, dtype=torch.float64, device="cuda") if has_ref and want_ref_risk else None
    ws, nws = None, 0
    if own_workspace:
        nws = _L().mdd_nbest_mbr_workspace_bytes(N, B, Cn, max_len)
        assert nws > 0 and nws % 16 == 0
        ws = torch.full((nws + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = _L().mdd_nbest_mbr(_ptr(d_ids), pitch, _ptr(d_nids), _ptr(d_st), _ptr(d_w), N, B, Cn, max_len, _ptr(d_ref), _ptr(d_rl),
                            ref.shape[1] if has_ref else 0, _ptr(best), _ptr(risk), _ptr(dist), _ptr(ref_dist), _ptr(ref_risk), _ptr(flag),
                            _ptr(ws), nws, None)
    torch.cuda.synchronize()
    assert rc == 0, _L().mdd_last_error().decode()
    if own_workspace:
        assert (ws[nws:] == 0x5A).all(), "the workspace was written past mdd_nbest_mbr_workspace_bytes"
    out = dict(best=best, risk=risk, flag=flag, dist=dist, ref_dist=ref_dist, ref_risk=ref_risk)
    out = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    assert (out["best"] != SENT_I).all() and (out["flag"] != SENT_I).all() and (out["risk"] != SENT_F).all(), "an output entry was not written"
    for k, sent in (("dist", SENT_I), ("ref_dist", SENT_I), ("ref_risk", SENT_F)):
        assert out[k] is None or (out[k] != sent).all(), "an entry of %s was not written" % k
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64) if a.dtype == np.float64 else a


def assert_same_bits(got, want, keys=("best", "risk", "flag", "dist", "ref_dist", "ref_risk"), tag=None):
    for k in keys:
        if got.get(k) is None or want.get(k) is None:
            continue
        assert got[k].shape == want[k].shape and (_bits(got[k]) == _bits(want[k])).all(), (tag, k)


# ----------------------------------------------------------------------------------------------------------------- the cases
# (name, N, B, C, max_len, exact lengths, id C - 1 present)
def _case(N, B, Cn, max_len, exact=None, top_id=False):
    exact = (max_len, 0, 1, max_len) if exact is None else exact
    return ("N%d_B%d_C%d_L%d" % (N, B, Cn, max_len), N, B, Cn, max_len, tuple(exact), top_id)


CASES = ([_case(N, 3, 45, 24) for N in (1, 2, 63, 64, 65)] + [_case(256, 3, 45, 20)] +
         [_case(5, 2, 45, L) for L in (1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] +
         [_case(9, 2, 2, 40), _case(9, 2, 2, 100), _case(9, 2, 256, 40, top_id=True), _case(9, 2, 256, 70, top_id=True)] +
         [_case(10, 1, 45, 30), _case(10, 70, 45, 30), _case(70, 70, 45, 12)])
BY_NAME = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(ids, nids, weights, ref, ref_len, yardstick) of a case: computed once, shared, never modified."""
    _, N, B, Cn, max_len, exact, top_id = BY_NAME[name]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    ids, nids = mr.draw_lists(seed, N, B, Cn, max_len, exact=exact[:N * B], top_id=top_id)
    ref, ref_len = mr.draw_lists(seed + 1, 1, B, Cn, max_len, pitch=max_len + 1)
    ref, ref_len = np.ascontiguousarray(ref[0]), np.ascontiguousarray(ref_len[0])
    if B > 1:
        ref_len[1] = 0                                   # an empty reference: the distance is the hypothesis' length
        ref[1] = 0
    w = mr.exact_weights(seed + 2, N, B)
    want = mr.reference(ids, nids, None, w, Cn, max_len, ref, ref_len)
    for a in (ids, nids, ref, ref_len, w):
        a.setflags(write=False)
    return ids, nids, w, ref, ref_len, want


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_distances_and_exact_risks_equal_the_yardstick(name):
    _, N, B, Cn, max_len, exact, top_id = BY_NAME[name]
    ids, nids, w, ref, ref_len, want = case_inputs(name)
    assert (want["flag"] == 0).all() and nids.max() == max_len and (nids == 0).any() == (N * B > 1)
    if top_id:
        assert (ids == Cn - 1).any()
    got = gpu_mbr(ids, nids, None, w, Cn, max_len, ref, ref_len)
    assert (got["dist"] == want["dist"]).all() and (got["ref_dist"] == want["ref_dist"]).all()
    assert_same_bits(got, want, tag=name)
    # structure: symmetric, zero diagonal, duplicates at distance 0, the empty reference at distance nids
    d = got["dist"]
    assert (d == d.transpose(0, 2, 1)).all() and (d[:, np.arange(N), np.arange(N)] == 0).all()
    for b in range(min(B, 3)):
        for n in range(N):
            for m in range(n):
                if nids[n, b] == nids[m, b] and (ids[n, b, :nids[n, b]] == ids[m, b, :nids[m, b]]).all():
                    assert d[b, n, m] == 0
    if B > 1:
        assert (got["ref_dist"][:, 1] == nids[:, 1]).all()


@pytest.mark.parametrize("name", ["N65_B3_C45_L24", "N5_B2_C45_L64", "N5_B2_C45_L129", "N9_B2_C256_L70", "N5_B2_C45_L1024"])
def test_poison_behind_the_lengths_changes_nothing(name):
    """2^30, -1 and valid ids behind every row's length, the reference row included: the outputs are bit-identical."""
    _, N, B, Cn, max_len, _, _ = BY_NAME[name]
    ids, nids, w, ref, ref_len, want = case_inputs(name)
    clean = gpu_mbr(ids, nids, None, w, Cn, max_len, ref, ref_len)
    dirty_ids = mr.poisoned(11, ids, nids, Cn)
    dirty_ref = mr.poisoned(12, ref[None], ref_len[None], Cn)[0]
    assert (dirty_ids == 2 ** 30).any() and (dirty_ids == -1).any() and (dirty_ref != ref).any()
    dirty = gpu_mbr(dirty_ids, nids, None, w, Cn, max_len, dirty_ref, ref_len)
    assert_same_bits(dirty, clean, tag=name)
    assert_same_bits(dirty, want, tag=name)


def _lists(rows, pitch=6):
    """ids [N,1,pitch] / nids [N,1] of one hand-made utterance."""
    ids, nids = np.zeros((len(rows), 1, pitch), dtype=np.int32), np.zeros((len(rows), 1), dtype=np.int32)
    for n, row in enumerate(rows):
        ids[n, 0, :len(row)], nids[n, 0] = row, len(row)
    return ids, nids


@pytest.mark.parametrize("rows,weights,best", [
    ([[1, 2, 3], [1, 2], [1, 2, 4], [1, 2]], [0.25, 0.25, 0.25, 0.25], 1),              # a duplicated hypothesis ties with itself: the lower rank
    ([[1, 2, 3], [1, 2], [1, 2, 4], [1, 2]], [0.5, 0.0, 0.5, 0.0], 0),                  # ranks 0 and 2 tie: the lower rank
    ([[1, 2], [3, 1, 2], [1, 2, 4], [1, 5, 2]], [0.0, 0.25, 0.25, 0.25], 1),            # the zero-weight row has the least risk and is not chosen
    ([[1, 2, 3, 4], [1, 2], [2]], [0.0, 0.0, 1.0], 2),                                  # all weight on one rank
    ([[7, 7, 7], [7, 7, 7], [7, 7, 7]], [0.125, 0.5, 0.375], 0),                        # a list that agrees with itself keeps rank 0
], ids=["duplicate", "tie", "zero_weight_least_risk", "one_rank", "all_agree"])
def test_tie_rule_on_constructed_lists(rows, weights, best):
    ids, nids = _lists(rows)
    w = np.array(weights, dtype=np.float64).reshape(-1, 1)
    want = mr.reference(ids, nids, None, w, 9, 6)
    assert want["best"][0] == best
    got = gpu_mbr(ids, nids, None, w, 9, 6)
    assert_same_bits(got, want)


@pytest.mark.parametrize("N", [64, 256])
def test_uniform_weights_at_a_power_of_two(N):
    """1 / N at N a power of two: exact products and sums, so risk is bit-equal in any order and the argmin is the yardstick's."""
    ids, nids = mr.draw_lists(500 + N, N, 2, 45, 20)
    w = np.full((N, 2), 1.0 / N)
    want = mr.reference(ids, nids, None, w, 45, 20)
    got = gpu_mbr(ids, nids, None, w, 45, 20)
    assert_same_bits(got, want)


@pytest.mark.parametrize("name", ["N2_B3_C45_L24", "N65_B3_C45_L24", "N256_B3_C45_L20", "N5_B2_C45_L513", "N70_B70_C45_L12"])
def test_softmax_weights_within_the_summation_bound(name):
    _, N, B, Cn, max_len, _, _ = BY_NAME[name]
    ids, nids, _, ref, ref_len, _ = case_inputs(name)
    w = mr.softmax_weights(77, N, B)
    assert (w == 0).any() or N < 5
    want = mr.reference(ids, nids, None, w, Cn, max_len, ref, ref_len)
    got = gpu_mbr(ids, nids, None, w, Cn, max_len, ref, ref_len)
    assert_same_bits(got, want, keys=("flag", "dist", "ref_dist"), tag=name)
    bound = N * 2.0 ** -52 * want["mass"]
    err = np.abs(got["risk"] - want["risk"])
    print("%s: max |risk - yardstick| %.3e, bound there %.3e" % (name, err.max(), bound.flat[err.argmax()]))
    assert (err <= bound).all(), (name, float((err - bound).max()))
    assert (np.abs(got["ref_risk"] - want["ref_risk"]) <= N * 2.0 ** -52 * want["ref_mass"]).all(), name
    decided = 0
    for b in range(B):
        k = got["best"][b]
        alive = np.nonzero(w[:, b] > 0)[0]
        assert k in alive, (name, b)
        lowest = want["risk"][alive, b].min()
        assert want["risk"][k, b] - lowest <= 2 * bound[k, b], (name, b)
        # Where every rank that does not tie with the yardstick's minimum exactly is further above it than the two sums may differ, the
        # argmin is decided: the yardstick's own.  An exact tie there is between copies of one hypothesis, whose terms and whose order of
        # summation are the same on the GPU too, so the tie rule -- the lower rank -- is pinned as well.
        kb = want["best"][b]
        others = alive[want["risk"][alive, b] != lowest]
        tied = alive[want["risk"][alive, b] == lowest]
        copies = all(nids[n, b] == nids[kb, b] and (ids[n, b, :nids[n, b]] == ids[kb, b, :nids[kb, b]]).all() for n in tied)
        if copies and (want["risk"][others, b] - lowest > bound[others, b] + bound[kb, b]).all():
            decided += 1
            assert k == kb, (name, b, k, kb)
    assert decided >= 1, "no utterance of the case has a decided argmin"


def test_flags_and_their_neighbours():
    """Utterances 1, 3, 5, 7, 9 are bad in five ways; the even ones are fine and must equal a run on the fine ones alone."""
    N, B, Cn, max_len = 12, 11, 45, 20
    ids, nids = mr.draw_lists(900, N, B, Cn, max_len, pitch=max_len + 2)
    ref, ref_len = mr.draw_lists(901, 1, B, Cn, max_len, pitch=max_len + 2)
    ref, ref_len = ref[0].copy(), ref_len[0].copy()
    w = mr.exact_weights(902, N, B)
    status = np.zeros(B, dtype=np.int32)
    status[1] = 2                                                       # skipped by status: its ids are poison and never looked at
    ids[:, 1] = 2 ** 30
    nids[:, 1] = 999
    w[:, 3] = 0.0                                                       # no weight above 0
    ids[4, 5, 0], nids[4, 5] = Cn, max(nids[4, 5], 1)                   # id = C inside a row
    ref[7, 2], ref_len[7] = -1, max(ref_len[7], 3)                      # id = -1 inside the reference row
    nids[N - 1, 9] = max_len + 1                                        # a length of max_len + 1 (inside the pitch)
    want = mr.reference(ids, nids, status, w, Cn, max_len, ref, ref_len)
    assert want["flag"].tolist() == [0, 1, 0, 1, 0, 2, 0, 2, 0, 2, 0]
    got = gpu_mbr(ids, nids, status, w, Cn, max_len, ref, ref_len)
    assert_same_bits(got, want)
    bad = want["flag"] != 0
    assert (got["best"][bad] == -1).all() and np.isnan(got["risk"][:, bad]).all() and np.isnan(got["ref_risk"][bad]).all()
    assert (got["dist"][bad] == -1).all() and (got["ref_dist"][:, bad] == -1).all()
    good = np.nonzero(~bad)[0]
    alone = gpu_mbr(np.ascontiguousarray(ids[:, good]), np.ascontiguousarray(nids[:, good]), None, np.ascontiguousarray(w[:, good]), Cn, max_len,
                    np.ascontiguousarray(ref[good]), np.ascontiguousarray(ref_len[good]))
    assert (alone["flag"] == 0).all()
    for k in ("best", "flag", "ref_risk"):
        assert (_bits(got[k][good]) == _bits(alone[k])).all(), k
    for k in ("risk", "ref_dist"):
        assert (_bits(np.ascontiguousarray(got[k][:, good])) == _bits(alone[k])).all(), k
    assert (got["dist"][good] == alone["dist"]).all()
    # a bad id wins over the weights; a status wins over everything
    w0 = w.copy()
    w0[:, 5] = 0.0
    assert gpu_mbr(ids, nids, status, w0, Cn, max_len, ref, ref_len)["flag"][5] == 2
    # the reference's length is also bounded by its own pitch
    short_ref = np.ascontiguousarray(ref[:, :4])
    rl = np.minimum(ref_len, 4)
    rl[0] = 5
    assert gpu_mbr(ids, nids, status, w, Cn, max_len, short_ref, rl)["flag"][0] == 2


@pytest.mark.parametrize("name", ["N65_B3_C45_L24", "N5_B2_C45_L257"])
def test_optional_outputs_workspace_and_repeat_runs_leave_the_bits_alone(name):
    _, N, B, Cn, max_len, _, _ = BY_NAME[name]
    ids, nids, _, ref, ref_len, _ = case_inputs(name)
    w = mr.softmax_weights(5, N, B)
    full = gpu_mbr(ids, nids, None, w, Cn, max_len, ref, ref_len)
    again = gpu_mbr(ids, nids, None, w, Cn, max_len, ref, ref_len)
    assert_same_bits(again, full, tag="two runs")
    assert_same_bits(gpu_mbr(ids, nids, None, w, Cn, max_len, ref, ref_len, want_dist=False), full, tag="dist NULL")
    assert_same_bits(gpu_mbr(ids, nids, None, w, Cn, max_len, ref, ref_len, want_ref_dist=False), full, tag="ref_dist NULL")
    assert_same_bits(gpu_mbr(ids, nids, None, w, Cn, max_len, ref, ref_len, want_ref_risk=False), full, tag="ref_risk NULL")
    assert_same_bits(gpu_mbr(ids, nids, None, w, Cn, max_len), full, keys=("best", "risk", "flag", "dist"), tag="no reference")
    assert_same_bits(gpu_mbr(ids, nids, np.zeros(B, dtype=np.int32), w, Cn, max_len, ref, ref_len), full, tag="status given")
    assert_same_bits(gpu_mbr(ids, nids, None, w, Cn, max_len, ref, ref_len, own_workspace=True), full, tag="caller workspace")


def test_hip_model_nbest_mbr_wrapper():
    from ctc_attention_mispronunciation_amd.hip_model import nbest_mbr
    name = "N10_B1_C45_L30"
    _, N, B, Cn, max_len, _, _ = BY_NAME[name]
    ids, nids, w, ref, ref_len, want = case_inputs(name)
    best, risk, flag, dist, ref_dist, ref_risk = nbest_mbr(torch.from_numpy(ids.copy()).cuda(), nids.copy(), None, w.copy(), Cn, ref=ref.copy(), ref_len=ref_len.copy(),
                                                           want_dist=True)
    assert best.is_cuda and risk.dtype == torch.float64 and tuple(dist.shape) == (B, N, N)
    got = dict(best=best, risk=risk, flag=flag, dist=dist, ref_dist=ref_dist, ref_risk=ref_risk)
    assert_same_bits({k: v.cpu().numpy() for k, v in got.items()}, want)
    best, risk, flag, dist, ref_dist, ref_risk = nbest_mbr(ids.copy(), nids.copy(), np.zeros(B, np.int32), w.copy(), Cn, max_len=max_len)
    assert dist is None and ref_dist is None and ref_risk is None and (best.cpu().numpy() == want["best"]).all()
    with pytest.raises(ValueError):
        nbest_mbr(ids.copy(), nids.copy(), None, w.copy(), Cn, ref=ref.copy())
    from ctc_attention_mispronunciation_amd._lib import MddError
    with pytest.raises(MddError, match="mdd_nbest_mbr.*max_len"):
        nbest_mbr(ids.copy(), nids.copy(), None, w.copy(), Cn, max_len=max_len + 100)


# ------------------------------------------------------------------------------------------------- BeamDecoder.decode_mbr
# Seed 1900 was chosen on the CPU: the yardstick beam of tests/nbest_reference.py, the oracle's CTC likelihood of each listed hypothesis,
# nbest_posteriors and mr.reference put the MBR hypothesis of utterance 0 at rank 9 of 10 (beam 10) and at rank 88 of 200 (beam 200), its
# risk 0.29 / 0.27 below the runner-up's; the other three utterances move too.  Both lists rank alike under the two exp flavours.
CHAIN_SEED, CHAIN_LENS = 1900, [40, 33, 40, 37]


def _chain_decoder(beam):
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    i2c = synth.phone_table_41()
    return BeamDecoder(i2c, beam_width=beam, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=0.2), i2c


def _chain_logp(T=40, B=4, Cn=45):
    from ctc_attention_mispronunciation_amd import synth
    return np.stack([synth.peaky_logp(T, Cn, max(1, T // 8) + b, seed=CHAIN_SEED + b) for b in range(B)], axis=1)


@pytest.mark.parametrize("beam", [10, 200])
def test_decode_mbr_is_the_yardstick_on_the_downloaded_list(beam):
    """Synthetic peaky posteriors at T = 40, B = 4, C = 45 through mdd_beam_nbest (beam 10) and mdd_beam_wide (beam 200): decode_mbr's
    records equal the yardstick run on the ids the search returned and the weights the rescoring gives them."""
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import nbest_posteriors
    T, B, Cn = 40, 4, 45
    dec, i2c = _chain_decoder(beam)
    assert _L().mdd_beam_fits(T, B, Cn, beam) == (1 if beam == 10 else 0)          # the two search entries
    lp = torch.from_numpy(_chain_logp(T, B, Cn)).cuda()
    rs = np.random.default_rng(3)
    canon_len = np.array([6, 9, 1, 7], dtype=np.int64)
    canon = rs.integers(1, Cn - 1, size=(B, 9)).astype(np.int64)
    got = dec.decode_mbr(lp, CHAIN_LENS, canonical_ids=torch.from_numpy(canon), canonical_lens=torch.from_numpy(canon_len))
    plain = dec.decode_mbr(lp, CHAIN_LENS)
    ids, nids, status, _ = dec.decode_nbest_ids(lp, CHAIN_LENS)
    ids_h, nids_h, status_h = ids.cpu().numpy(), nids.cpu().numpy(), status.cpu().numpy()
    N = ids_h.shape[0]
    assert N == beam and (status_h == 0).all()
    ll = dec.nbest_loglik(lp, CHAIN_LENS, ids, nids, max_len=int(nids_h.max()))
    w = np.stack([nbest_posteriors(ll[:, b]) for b in range(B)], axis=1)
    want = mr.reference(ids_h, nids_h, status_h, w, Cn, max(int(nids_h.max()), int(canon_len.max())), canon.astype(np.int32), canon_len.astype(np.int32))
    assert (want["flag"] == 0).all()
    bound = N * 2.0 ** -52 * want["mass"]
    for b in range(B):
        string, rank, risk, risk0, exp = got[b]
        risks = np.sort(want["risk"][w[:, b] > 0, b])
        assert risks[1] - risks[0] > 4 * bound[:, b].max(), "the case's argmin hangs on the rounding of a sum"
        k = int(want["best"][b])
        assert rank == k and string == " ".join(i2c[i] for i in ids_h[k, b, :nids_h[k, b]]), (beam, b, rank, k)
        assert abs(risk - want["risk"][k, b]) <= bound[k, b] and abs(risk0 - want["risk"][0, b]) <= bound[0, b], (beam, b)
        assert abs(exp - want["ref_risk"][b]) <= N * 2.0 ** -52 * want["ref_mass"][b], (beam, b)
        assert risk <= risk0
        assert plain[b] == (string, rank, risk, risk0, None)
    assert got[0][1] != 0, "utterance 0's MBR hypothesis must not be the 1-best (see CHAIN_SEED)"
    print("beam %d: MBR ranks %s, risk / risk of rank 0 %s" % (beam, [r[1] for r in got], [(round(r[2], 4), round(r[3], 4)) for r in got]))


def test_decode_mbr_raises_what_decode_raises_and_names_the_limit():
    dec, _ = _chain_decoder(10)
    lp = torch.from_numpy(_chain_logp()).cuda()
    with pytest.raises(IndexError):
        dec.decode(lp, [40, 0, 40, 40])
    with pytest.raises(IndexError):
        dec.decode_mbr(lp, [40, 0, 40, 40])
    with pytest.raises(ValueError, match="nbest must be"):
        dec.decode_mbr(lp, CHAIN_LENS, nbest=11)
    long_canon = torch.ones((4, 1030), dtype=torch.int64)
    with pytest.raises(ValueError, match="1024"):
        dec.decode_mbr(lp, CHAIN_LENS, canonical_ids=long_canon, canonical_lens=torch.tensor([5, 5, 1025, 5]))
    got = dec.decode_mbr(lp, CHAIN_LENS, nbest=2)
    assert all(r is not None and r[1] in (0, 1) for r in got)


def test_decode_mbr_with_a_canonical_longer_than_the_frames():
    """A canonical row of more ids than the T frames a hypothesis row holds (max_len bounds both, and it may not pass the rows' pitch):
    decode_mbr widens the rows instead of failing, and the figures are the yardstick's on the list as the search returned it."""
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import nbest_posteriors
    T, B, Cn = 12, 2, 45
    dec, i2c = _chain_decoder(10)
    lp = torch.from_numpy(_chain_logp(T, B, Cn)).cuda()
    lens = [12, 10]
    canon_len = np.array([T + 5, 3], dtype=np.int64)
    canon = np.random.default_rng(4).integers(1, Cn - 1, size=(B, T + 7)).astype(np.int64)
    got = dec.decode_mbr(lp, lens, canonical_ids=torch.from_numpy(canon), canonical_lens=torch.from_numpy(canon_len))
    ids, nids, status, _ = dec.decode_nbest_ids(lp, lens)
    ids_h, nids_h = ids.cpu().numpy(), nids.cpu().numpy()
    assert ids_h.shape[2] == T < canon_len.max()
    ll = dec.nbest_loglik(lp, lens, ids, nids, max_len=int(nids_h.max()))
    w = np.stack([nbest_posteriors(ll[:, b]) for b in range(B)], axis=1)
    wide = np.zeros(ids_h.shape[:2] + (T + 5,), dtype=np.int32)
    wide[:, :, :T] = ids_h
    want = mr.reference(wide, nids_h, status.cpu().numpy(), w, Cn, T + 5, canon.astype(np.int32), canon_len.astype(np.int32))
    assert (want["flag"] == 0).all()
    N = ids_h.shape[0]
    for b in range(B):
        assert got[b] is not None
        string, rank, risk, risk0, exp = got[b]
        assert abs(exp - want["ref_risk"][b]) <= N * 2.0 ** -52 * want["ref_mass"][b] and exp >= canon_len[b] - nids_h[:, b].max()
        assert abs(risk - want["risk"][rank, b]) <= N * 2.0 ** -52 * want["mass"][rank, b]
        assert want["risk"][rank, b] - want["risk"][want["best"][b], b] <= 2 * N * 2.0 ** -52 * want["mass"][rank, b]
        assert string == " ".join(i2c[i] for i in ids_h[rank, b, :nids_h[rank, b]])
