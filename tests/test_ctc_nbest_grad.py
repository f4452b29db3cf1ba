"""mdd_ctc_nbest_grad and mdd_nbest_risk (csrc/ctc_nbest_grad.hip) on the GPU.

The gradient is held to the float64 yardstick of tests/ctc_nbest_grad_cases.py (CPU ``torch.nn.functional.ctc_loss`` on a double leaf, one
call per rank, under autograd): per utterance ``|grad - f64| <= GRAD_ATOL sum_n |coef[n,b]|`` with the 5e-6 tests/ctc_loss_cases.py holds
mdd_ctc_loss's wave forms to (the output is a linear combination of tensors each held to that bound), and the sum over the classes of a live
frame ``<= CLASS_SUM sum_n |coef[n,b]|`` (1e-4, same file).  Shapes are the smallest at which the kernel takes another path: every labels-
per-lane count, one group and several (csrc/plan.h's ctc_nbest_grad_plan spreads the ranks over 256 / B groups, so B decides: B = 2 gives a
group per rank, B = 100 two groups with a partial last one, B = 300 one group that runs every rank), the LDS bound, and the edge rows.
With N = 1 and coef = 1 the output has the BITS of ``hip_model.ctc_loss``'s gradient (the kernel restates ctc_wave_kernel's arithmetic and
adds 1.f * exp(lp) + (0.f - occupancy)); the test asserts that, which is stronger than the 2 GRAD_ATOL it would otherwise be held to."""
import functools

import numpy as np
import pytest
import torch

from tests import ctc_nbest_cases as cc
from tests import ctc_nbest_grad_cases as gc
from tests.helpers import record_margin

pytestmark = pytest.mark.gpu
_WORST = {"grad": 0.0, "class_sum": 0.0}


def _cuda(*arrays):
    return tuple(torch.from_numpy(np.array(a)).cuda() for a in arrays)


def _run(lp, lens, ids, nids, coef, blank=0, max_len=None, want_loglik=False):
    from ctc_attention_mispronunciation_amd import hip_model
    d = _cuda(lp, lens, ids, nids, coef)
    grad, flag, ll = hip_model.ctc_nbest_grad(*d, blank=blank, max_len=max_len, want_loglik=want_loglik)
    assert grad.dtype == torch.float32 and grad.is_cuda and tuple(grad.shape) == tuple(lp.shape) and flag.dtype == torch.int32
    return grad.cpu().numpy(), flag.cpu().numpy(), None if ll is None else ll.cpu().numpy()


def _hold(tag, grad, ref, coef, lens):
    """The two bounds per utterance, rows >= len exactly zero; the worst ratios go to the margins file."""
    T = grad.shape[0]
    atol, csum = gc.utterance_bounds(coef)
    for b in range(grad.shape[1]):
        Tb = int(np.clip(lens[b], 0, T))
        assert (grad[Tb:, b] == 0).all(), (tag, b)
        err = float(np.abs(grad[:, b].astype(np.float64) - ref[:, b]).max())
        cs = float(np.abs(grad[:Tb, b].astype(np.float64).sum(axis=-1)).max(initial=0.0))
        print("%s b %d: |grad - f64| %.3e (bound %.3e), |class sum| %.3e (bound %.3e)" % (tag, b, err, atol[b], cs, csum[b]))
        if atol[b] > 0:
            _WORST["grad"], _WORST["class_sum"] = max(_WORST["grad"], err / atol[b]), max(_WORST["class_sum"], cs / csum[b])
        record_margin("ctc_nbest_grad_abs_over_bound", _WORST["grad"], 1.0)
        record_margin("ctc_nbest_grad_class_sum_over_bound", _WORST["class_sum"], 1.0)
        assert err <= atol[b] and cs <= csum[b], (tag, b, err, atol[b], cs, csum[b])


def _case_and_ref(seed, T, B, Cn, N, longest, blank=0, scale=2.0, lens=None):
    lp = cc.dense_logp(seed, T, B, Cn, scale=scale)
    ids, nids = gc.no_repeat_lists(seed + 1, N, B, Cn, blank, longest, pitch=max(longest, 1) + 3)
    coef = gc.draw_coef(seed + 2, N, B)
    lens = np.full((B,), T, dtype=np.int32) if lens is None else np.asarray(lens, dtype=np.int32)
    return lp, lens, ids, nids, coef


# --------------------------------------------------------------------------------------------------------------------- tiny
@functools.lru_cache(maxsize=None)
def _tiny(blank):
    """B = 3, T = 12, C = 5, N = 4: one empty hypothesis, and in the utterance of four frames a repeat that needs five, with coef 0."""
    lp, lens, ids, nids, coef = _case_and_ref(3200 + blank, 12, 3, 5, 4, 4, blank=blank, lens=(12, 9, 4))
    nids[1, 0] = 0
    k = 1 if blank != 1 else 2
    ids[3, 2, :3], nids[3, 2], coef[3, 2] = (k, k, k), 3, 0.0
    ref = gc.weighted_grad_f64(lp, lens, ids, nids, coef, blank=blank, max_len=4)
    return lp, lens, ids, nids, coef, ref


@pytest.mark.parametrize("blank", [0, 2, 4])
def test_tiny_with_an_empty_and_a_skipped_infeasible_hypothesis(blank):
    lp, lens, ids, nids, coef, ref = _tiny(blank)
    assert np.isinf(gc.nll_f64(lp, lens, ids, nids, blank, 4)[3, 2])
    grad, flag, ll = _run(lp, lens, ids, nids, coef, blank=blank, max_len=4, want_loglik=True)
    assert (flag == 0).all() and np.isnan(ll[3, 2]) and np.isfinite(np.delete(ll.reshape(-1), 3 * 3 + 2)).all()
    _hold("tiny blank %d" % blank, grad, ref, coef, lens)


# -------------------------------------------------------------------------------------------------- labels per lane, groups
@pytest.mark.parametrize("longest", [63, 64, 127, 128, 255])
def test_where_the_scan_changes_its_labels_per_lane(longest):
    T, B, Cn, N = longest + 24, 2, 8, 3
    assert gc.plan(T, B, Cn, N, longest).NL == (1 if longest <= 63 else 2 if longest <= 127 else 4)
    lp, lens, ids, nids, coef = _case_and_ref(3300 + longest, T, B, Cn, N, longest, lens=(T, T - 5))
    assert int(nids[0, 0]) == longest
    grad, flag, _ = _run(lp, lens, ids, nids, coef, max_len=longest)
    assert (flag == 0).all()
    _hold("lanes L%d" % longest, grad, gc.weighted_grad_f64(lp, lens, ids, nids, coef, max_len=longest), coef, lens)


@pytest.mark.parametrize("N,B", [(1, 2), (4, 2), (5, 2), (10, 2), (11, 2), (17, 2), (256, 2), (5, 100), (11, 100), (17, 300), (4, 64)])
def test_rank_grouping(N, B):
    """B = 2: a group per rank (N = 256: two ranks a group); B = 100: two groups, the last one partial; B = 300: one group runs every rank
    and stores the rows itself; B = 64: four groups of one."""
    T, Cn, longest = 16, 6, 5
    p = gc.plan(T, B, Cn, N, longest)
    assert (p.ranks, p.groups) == {(256, 2): (2, 128), (5, 100): (3, 2), (11, 100): (6, 2), (17, 300): (17, 1), (4, 64): (1, 4)}.get((N, B), (1, N)), p
    lp, lens, ids, nids, coef = _case_and_ref(3400 + N + B, T, B, Cn, N, longest, lens=[T - (b % 4) for b in range(B)])
    grad, flag, _ = _run(lp, lens, ids, nids, coef, max_len=longest)
    assert (flag == 0).all()
    _hold("groups N%d B%d" % (N, B), grad, gc.weighted_grad_f64(lp, lens, ids, nids, coef, max_len=longest), coef, lens)


@pytest.mark.parametrize("B", [2, 100, 300])
def test_every_second_coefficient_zero(B):
    T, Cn, N, longest = 16, 6, 10, 5
    lp, lens, ids, nids, coef = _case_and_ref(3500 + B, T, B, Cn, N, longest)
    coef[1::2] = 0.0
    ids[1::2] = 1 << 20                      # whatever a skipped rank's ids are
    grad, flag, ll = _run(lp, lens, ids, nids, coef, max_len=longest, want_loglik=True)
    assert (flag == 0).all() and np.isnan(ll[1::2]).all() and np.isfinite(ll[0::2]).all()
    _hold("alternate B%d" % B, grad, gc.weighted_grad_f64(lp, lens, ids[0::2], nids[0::2], coef[0::2], max_len=longest), coef, lens)


# ------------------------------------------------------------------------------------------------------------------ lengths
def test_lengths_zero_short_and_clamped():
    from ctc_attention_mispronunciation_amd import hip_model
    T, B, Cn, N, longest = 16, 4, 6, 3, 5
    lens = np.array([0, 7, T + 5, T], dtype=np.int32)
    lp, _, ids, nids, coef = _case_and_ref(3600, T, B, Cn, N, longest)
    nids[1, 0] = 0                           # an empty hypothesis of the utterance without frames: log-likelihood 0
    grad, flag, ll = _run(lp, lens, ids, nids, coef, max_len=longest, want_loglik=True)
    want_ll = hip_model.ctc_nbest(*_cuda(lp, lens, ids, nids), max_len=longest).cpu().numpy()
    assert np.array_equal(ll.view(np.int64), want_ll.view(np.int64)) and ll[1, 0] == 0 and np.isneginf(ll[0, 0])
    assert flag.tolist() == [1, 0, 0, 0] and (grad[:, 0] == 0).all() and (grad[7:, 1] == 0).all() and np.abs(grad[:7, 1]).max() > 1e-3
    ref = gc.weighted_grad_f64(lp, np.clip(lens, 0, T), ids, nids, coef, max_len=longest)
    ref[:, 0] = 0
    _hold("lengths", grad, ref, coef, lens)
    # without frames and with empty hypotheses only, nothing is wrong with the utterance
    nids0 = nids.copy()
    nids0[:, 0] = 0
    grad0, flag0, _ = _run(lp, lens, ids, nids0, coef, max_len=longest)
    assert flag0.tolist() == [0, 0, 0, 0] and (grad0[:, 0] == 0).all() and np.array_equal(grad0[:, 1:], grad[:, 1:])


def test_the_lds_bound_itself():
    from ctc_attention_mispronunciation_amd import _lib, hip_model
    Cn, longest = 45, 14
    T = gc.tmax(Cn, longest)
    assert hip_model.ctc_nbest_grad_fits(T, Cn, longest) and not hip_model.ctc_nbest_grad_fits(T + 1, Cn, longest) and gc.plan(T, 1, Cn, 2, longest).smem <= gc.LDS_MAX
    lp, lens, ids, nids, coef = _case_and_ref(3700, T, 1, Cn, 2, longest)
    grad, flag, _ = _run(lp, lens, ids, nids, coef, max_len=longest)
    assert (flag == 0).all()
    _hold("lds edge T%d" % T, grad, gc.weighted_grad_f64(lp, lens, ids, nids, coef, max_len=longest), coef, lens)
    with pytest.raises(_lib.MddError, match="mdd_ctc_nbest_grad.*LDS"):
        hip_model.ctc_nbest_grad(torch.zeros((T + 1, 1, Cn), device="cuda"), [T + 1], *_cuda(ids, nids, coef), max_len=longest)


@pytest.mark.parametrize("scale,blank", [(30.0, 0), (12.0, 44)])
def test_peaked_log_probs(scale, blank):
    """Log-probs down to -190 (about -210 at B = 3 there), at the shape and scales tests/ctc_loss_cases.py draws its peaked cases (T = 250, C = 45, 40 labels)."""
    T, B, Cn, N, longest = 250, 2, 45, 4, 40
    lp, lens, ids, nids, coef = _case_and_ref(3800 + blank, T, B, Cn, N, longest, blank=blank, scale=scale, lens=(T, 201))
    assert lp.min() < (-180 if scale == 30.0 else -80)
    grad, flag, _ = _run(lp, lens, ids, nids, coef, blank=blank, max_len=longest)
    assert (flag == 0).all()
    _hold("peaked x%g" % scale, grad, gc.weighted_grad_f64(lp, lens, ids, nids, coef, blank=blank, max_len=longest), coef, lens)


# -------------------------------------------------------------------------------------------------------------------- flags
@pytest.mark.parametrize("B", [3, 100])
def test_flags_zero_the_utterance_and_leave_its_neighbours_their_bits(B):
    """Flag 1: a live rank that is no path.  Flag 2: a live rank with a label outside the classes; a coef that is not finite.  A bad id in a
    rank with coef 0 is no flag.  B = 3: a group per rank; B = 100: groups of several ranks."""
    T, Cn, N, longest = 16, 6, 6, 5
    lp, lens, ids, nids, coef = _case_and_ref(3900 + B, T, B, Cn, N, longest)
    clean, flag, ll_clean = _run(lp, lens, ids, nids, coef, max_len=longest, want_loglik=True)
    assert (flag == 0).all()
    lens2, ids2, coef2 = lens.copy(), ids.copy(), coef.copy()
    lens2[0] = 4
    ids2[2, 0, :3], nids2 = (3, 3, 3), nids.copy()
    nids2[2, 0] = 3                                        # 3 3 3 in four frames: no path
    ids2[4, 1, 1] = Cn                                     # a label outside the classes
    ids2[5, 2, 0], coef2[5, 2] = -7, 0.0                   # a bad id where coef is 0: not scanned, not flagged
    grad, flag, ll = _run(lp, lens2, ids2, nids2, coef2, max_len=longest, want_loglik=True)
    assert flag[:3].tolist() == [1, 2, 0] and (flag[3:] == 0).all()
    assert (grad[:, :2] == 0).all() and np.isneginf(ll[2, 0]) and np.isnan(ll[4, 1]) and np.isnan(ll[5, 2])
    assert np.array_equal(grad[:, 3:].view(np.int32), clean[:, 3:].view(np.int32))
    keep = np.ones((N, B), dtype=bool)
    keep[:, 0], keep[4, 1], keep[5, 2] = False, False, False
    assert np.array_equal(ll[keep].view(np.int64), ll_clean[keep].view(np.int64))      # the other ranks of a flagged utterance are still scanned
    ref = gc.weighted_grad_f64(lp, lens, ids, nids, coef2, max_len=longest)
    err = np.abs(grad[:, 2].astype(np.float64) - ref[:, 2]).max()
    assert err <= gc.utterance_bounds(coef2)[0][2]
    for v in (np.inf, np.nan):
        coef3 = coef.copy()
        coef3[3, 1] = v
        grad, flag, _ = _run(lp, lens, ids, nids, coef3, max_len=longest)
        assert flag[:3].tolist() == [0, 2, 0] and (grad[:, 1] == 0).all()
        assert np.array_equal(np.delete(grad, 1, axis=1).view(np.int32), np.delete(clean, 1, axis=1).view(np.int32))


# ------------------------------------------------------------------------------------------------------- loglik, bits, memory
def test_loglik_has_the_bits_of_ctc_nbest():
    from ctc_attention_mispronunciation_amd import hip_model
    case = cc.ragged("peaky")
    N, B = 19, 3
    coef = gc.draw_coef(4000, N, B)
    coef[3] = 0.0
    lp, lens, ids, nids = (np.array(a) for a in (case.lp, case.lens, case.ids[:N], case.nids[:N]))
    _, _, ll = _run(lp, lens, ids, nids, coef, max_len=case.max_len, want_loglik=True)
    want = hip_model.ctc_nbest(*_cuda(lp, lens, ids, nids), max_len=case.max_len).cpu().numpy()
    live = coef != 0
    assert np.array_equal(ll[live].view(np.int64), want[live].view(np.int64)) and np.isnan(ll[~live]).all() and np.isfinite(want).any()


def _raw(lp, lens, ids, nids, coef, max_len, grad, flag, ws, ws_bytes, blank=0):
    from ctc_attention_mispronunciation_amd import _lib
    T, B, Cn = lp.shape
    N, _, pitch = ids.shape
    p = _lib.ptr
    return _lib.lib().mdd_ctc_nbest_grad(p(lp), T, B, Cn, p(lens), p(ids), pitch, p(nids), N, max_len, blank, p(coef), None, p(grad), p(flag), p(ws), ws_bytes,
                                         _lib.current_stream_ptr())


@pytest.mark.parametrize("B", [2, 300])
def test_repeatability_and_the_callers_workspace(B):
    from ctc_attention_mispronunciation_amd import _lib
    T, Cn, N, longest = 16, 6, 11, 5
    lp, lens, ids, nids, coef = _case_and_ref(4100 + B, T, B, Cn, N, longest)
    first, _, _ = _run(lp, lens, ids, nids, coef, max_len=longest)
    again, _, _ = _run(lp, lens, ids, nids, coef, max_len=longest)
    assert np.array_equal(first.view(np.int32), again.view(np.int32)) and np.abs(first).max() > 1e-3
    need = _lib.lib().mdd_ctc_nbest_grad_workspace_bytes(T, B, Cn, N, longest)
    assert need == gc.plan(T, B, Cn, N, longest).bytes
    d = _cuda(lp, lens, ids, nids, coef)
    spare = 64
    ws = torch.full((need + spare,), 0x5a, dtype=torch.uint8, device="cuda")
    grad = torch.full((T * B * Cn + spare,), -7.0, dtype=torch.float32, device="cuda")
    flag = torch.full((B + spare,), -7, dtype=torch.int32, device="cuda")
    assert _raw(*d, longest, grad, flag, ws, need) == 0
    torch.cuda.synchronize()
    assert np.array_equal(grad[:T * B * Cn].cpu().numpy().view(np.int32), first.reshape(-1).view(np.int32))
    assert bool((grad[T * B * Cn:] == -7.0).all()) and bool((flag[B:] == -7).all()) and bool((flag[:B] == 0).all()) and bool((ws[need:] == 0x5a).all())
    assert _raw(*d, longest, grad, flag, ws, need - 1) == -1
    msg = _lib.lib().mdd_last_error().decode()
    assert msg.startswith("mdd_ctc_nbest_grad") and "workspace_bytes" in msg, msg


@pytest.mark.parametrize("longest", [12, 100, 200])
def test_one_rank_with_coefficient_one_has_the_bits_of_ctc_loss(longest):
    from ctc_attention_mispronunciation_amd import hip_model
    T, B, Cn = longest + 20, 3, 9
    lp, lens, ids, nids, _ = _case_and_ref(4200 + longest, T, B, Cn, 1, longest, lens=(T, T - 3, T - 7))
    grad, flag, _ = _run(lp, lens, ids, nids, np.ones((1, B)), max_len=longest)
    d = _cuda(lp, lens, ids, nids)
    _, want = hip_model.ctc_loss(d[0], d[2][0, :, :longest], d[1], d[3][0], want_grad=True)
    want = want.cpu().numpy()
    assert (flag == 0).all() and np.abs(grad - want).max() <= 2 * gc.GRAD_ATOL
    assert np.array_equal(grad.view(np.int32), want.view(np.int32))


# --------------------------------------------------------------------------------------------------------------------- risk
def _risk_numpy(loglik, cost, status=None):
    N, B = loglik.shape
    post, coef, risk, flag = np.zeros((N, B)), np.zeros((N, B)), np.full((B,), np.nan), np.zeros((B,), dtype=np.int32)
    for b in range(B):
        fin = np.isfinite(loglik[:, b])
        flag[b] = 1 if status is not None and status[b] != 0 else 2 if (cost[:, b] < 0).any() else 1 if not fin.any() else 0
        if flag[b]:
            continue
        e = np.where(fin, np.exp(np.where(fin, loglik[:, b], 0.0) - loglik[fin, b].max()), 0.0)
        post[:, b] = e / e.sum()
        risk[b] = (post[:, b] * cost[:, b]).sum()
        coef[:, b] = post[:, b] * (risk[b] - cost[:, b])
    return post, risk, coef, flag


@pytest.mark.parametrize("N", [1, 2, 10, 64, 65, 256])
def test_nbest_risk_against_numpy(N):
    """Columns: ordinary, some ranks -inf and NaN, all ranks -inf, status != 0, a cost of -1, ordinary again."""
    from ctc_attention_mispronunciation_amd import hip_model
    rs = np.random.default_rng(4300 + N)
    B = 6
    loglik = -rs.uniform(20.0, 60.0, size=(N, B))
    cost = rs.integers(0, 12, size=(N, B)).astype(np.int32)
    loglik[::3, 1] = -np.inf
    loglik[1::3, 1] = np.nan
    if N < 3:
        loglik[:, 1] = (-np.inf, -30.0)[:N] if N == 2 else np.nan
    loglik[:, 2] = -np.inf
    status = np.array([0, 0, 0, 3, 0, 0], dtype=np.int32)
    cost[N // 2, 4] = -1
    want = _risk_numpy(loglik, cost, status)
    got = [t.cpu().numpy() for t in hip_model.nbest_risk(torch.from_numpy(loglik).cuda(), torch.from_numpy(cost).cuda(), torch.from_numpy(status).cuda())]
    assert got[3].tolist() == want[3].tolist() == [0, 1 if N == 1 else 0, 1, 1, 2, 0]
    for g, w, name in zip(got[:3], want[:3], ("post", "risk", "coef")):
        assert np.array_equal(np.isnan(g), np.isnan(w)), name
        scale = np.abs(w[np.isfinite(w)]).max(initial=1e-300)
        assert np.nanmax(np.abs(g - w), initial=0.0) <= 1e-12 * max(scale, 1.0), (name, np.nanmax(np.abs(g - w)))
    fl = want[3] != 0
    assert (got[0][:, fl] == 0).all() and (got[2][:, fl] == 0).all() and np.isnan(got[1][fl]).all()
    assert np.abs(got[2][:, ~fl].sum(axis=0)).max() <= 1e-12
    if N == 1:
        assert (got[2] == 0).all() and (got[0][:, [0, 5]] == 1).all()
    # without a status array, and repeatable to the bit
    no_status = [t.cpu().numpy() for t in hip_model.nbest_risk(torch.from_numpy(loglik).cuda(), torch.from_numpy(cost).cuda())]
    assert no_status[3][3] == 0 and np.array_equal(np.delete(no_status[2], 3, axis=1), np.delete(got[2], 3, axis=1))
