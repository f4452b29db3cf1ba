"""The host side of MWER training (csrc/ctc_nbest_grad.hip, train.MWERLoss, steps/train_ctc.py), without a GPU.

  * the float64 yardstick of tests/ctc_nbest_grad_cases.py against itself: autograd's d risk / d nll is the closed form P (R - cost) to
    1e-12, the coefficients of an utterance sum to zero, the two forms of the gradient agree, and the gradient agrees with central finite
    differences of the risk on one tiny case;
  * csrc/plan.h's ctc_nbest_grad_plan with the host compiler: LDS within a CU, the grid covers N, NL is ctc_labels_per_lane, the workspace
    formula is the library's mdd_ctc_nbest_grad_workspace_bytes, the training shape (250, 45, 255) fits;
  * the symbols are declared, listed and exported; every refusal of the entries: MDD_ERR_ARG before any device work (the pointers are fake
    and never dereferenced), the message starting with the entry's name and naming the argument;
  * the conf checks of steps.train_ctc: the four status-2 refusals, each by its message, before data or device are touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ctc_nbest_cases as cc
from tests import ctc_nbest_grad_cases as gc
from tests.helpers import GOLD, ROOT

MDD_ERR_ARG = -1
_FAKE = 4096      # a non-NULL value for pointers that must never be dereferenced: every call below is refused on the host
KB = 1024


def _L():
    from ctc_attention_mispronunciation_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------ the yardstick
def _tiny():
    """T = 6, C = 4, N = 3, B = 2: short hypotheses, one with a repeat; costs as edit distances would be."""
    lp = cc.dense_logp(3100, 6, 2, 4, scale=1.0)
    ids = np.array([[[1, 2, 0], [3, 0, 0]], [[1, 1, 0], [3, 2, 0]], [[2, 0, 0], [1, 2, 3]]], dtype=np.int32)
    nids = np.array([[2, 1], [2, 2], [1, 3]], dtype=np.int32)
    cost = np.array([[0, 2], [1, 0], [3, 1]], dtype=np.int32)
    return lp, np.array([6, 5], dtype=np.int32), ids, nids, cost


def test_autograd_coefficients_are_the_closed_form():
    lp, lens, ids, nids, cost = _tiny()
    r = gc.risk_f64(lp, lens, ids, nids, cost, max_len=3)
    assert np.isfinite(r.nll).all() and np.allclose(r.post.sum(axis=0), 1.0, atol=1e-14)
    assert np.abs(r.autograd_coef - r.coef).max() <= 1e-12
    assert np.abs(r.coef.sum(axis=0)).max() <= 1e-12 and np.abs(r.coef).max() > 1e-3
    # the linear form with those coefficients is the same tensor
    lin = gc.weighted_grad_f64(lp, lens, ids, nids, r.coef, max_len=3)
    assert np.abs(lin - r.grad).max() <= 1e-12 and np.abs(r.grad).max() > 1e-3
    assert (r.grad[5:, 1] == 0).all()                      # the frame behind len


def test_a_rank_that_is_no_path_has_posterior_zero_and_leaves_the_rest_alone():
    lp, lens, ids, nids, cost = _tiny()
    ids, nids = ids.copy(), nids.copy()
    ids[1, 1, :3], nids[1, 1] = (2, 2, 2), 3               # 2 2 2 needs five frames and a blank between any two: utterance 1 has five -- feasible
    ids[2, 0, :3], nids[2, 0] = (3, 3, 3), 3
    lens = np.array([4, 5], dtype=np.int32)                # utterance 0 has four frames: 3 3 3 is no path
    r = gc.risk_f64(lp, lens, ids, nids, cost, max_len=3)
    assert np.isinf(r.nll[2, 0]) and np.isfinite(np.delete(r.nll.reshape(-1), 4)).all()
    assert r.post[2, 0] == 0 and r.coef[2, 0] == 0 and abs(r.post[:, 0].sum() - 1) <= 1e-14
    assert np.abs(r.autograd_coef - r.coef).max() <= 1e-12 and np.isfinite(r.grad).all()
    two = gc.risk_f64(lp, lens, ids[:2], nids[:2], cost[:2], max_len=3)
    assert np.abs(two.grad[:, 0] - r.grad[:, 0]).max() <= 1e-14


def test_yardstick_against_central_finite_differences():
    """d (sum_b risk_b) / d lp[t,b,c] with lp an independent variable: the coefficients sum to zero, so ATen's exp(lp) terms cancel and the
    deposited tensor is the plain derivative."""
    lp, lens, ids, nids, cost = _tiny()
    r = gc.risk_f64(lp, lens, ids, nids, cost, max_len=3)

    def total(x):
        nll = gc.nll_f64(x, lens, ids, nids, max_len=3)
        p = np.exp(-nll - (-nll).max(axis=0))
        p = p / p.sum(axis=0)
        return float((p * cost).sum())

    x0, h, worst = lp.astype(np.float64), 1e-5, 0.0
    assert abs(total(x0) - r.risk.sum()) <= 1e-12
    for t in range(6):
        for b in range(2):
            for c in range(4):
                xp, xm = x0.copy(), x0.copy()
                xp[t, b, c] += h
                xm[t, b, c] -= h
                worst = max(worst, abs((total(xp) - total(xm)) / (2 * h) - r.grad[t, b, c]))
    assert worst <= 1e-8, worst


# -------------------------------------------------------------------------------------------------------------------- plan
def test_plan_on_the_host_and_the_librarys_answers():
    L = _L()
    r = subprocess.run([gc.plan_driver()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "; 0 mismatch(es)" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"accepted (\d+) shapes; largest LDS of a workgroup: (\d+) bytes", r.stdout)
    assert int(m.group(1)) > 5000 and int(m.group(2)) <= gc.LDS_MAX
    tm = {(int(a), int(b)): int(c) for a, b, c in (line.split()[1:] for line in r.stdout.splitlines() if line.startswith("tmax "))}
    assert len(tm) == 9 and tm[(45, 255)] >= 250
    for (Cn, max_len), T in tm.items():
        assert L.mdd_ctc_nbest_grad_fits(T, Cn, max_len) == 1 and L.mdd_ctc_nbest_grad_fits(T + 1, Cn, max_len) == 0, (Cn, max_len, T)
        assert L.mdd_ctc_nbest_fits(T, Cn, max_len) == 1 and gc.tmax(Cn, max_len) == T
    assert L.mdd_ctc_nbest_grad_fits(250, 45, 255) == 1 and L.mdd_ctc_nbest_grad_fits(250, 45, 256) == 0
    from ctc_attention_mispronunciation_amd import hip_model
    assert hip_model.ctc_nbest_grad_fits(250, 45, 255) is True and hip_model.ctc_nbest_grad_fits(tm[(45, 255)] + 1, 45, 255) is False


@pytest.mark.parametrize("T,B,Cn,N,max_len", [(250, 32, 45, 10, 64), (250, 32, 45, 100, 40), (12, 3, 5, 4, 4), (16, 2, 6, 256, 5), (279, 2, 8, 3, 255),
                                             (40, 300, 45, 7, 10), (70, 1, 256, 256, 127)])
def test_workspace_bytes_are_the_plans(T, B, Cn, N, max_len):
    p = gc.plan(T, B, Cn, N, max_len)
    assert p.fits and p.smem <= gc.LDS_MAX and p.groups * p.ranks >= N > (p.groups - 1) * p.ranks
    assert p.NL == (1 if max_len <= 63 else 2 if max_len <= 127 else 4) == cc.plan(T, B, Cn, N, max_len).NL
    assert p.bytes == p.rows_bytes + p.slab_bytes + p.flag_bytes and p.rows_bytes == 8 * p.groups * B * 2 * T * 2 * (max_len + 1)
    assert (p.slab_bytes, p.flag_bytes) == ((4 * p.groups * T * B * Cn, 4 * p.groups * B) if p.groups > 1 else (0, 0))
    assert _L().mdd_ctc_nbest_grad_workspace_bytes(T, B, Cn, N, max_len) == p.bytes


def test_workspace_bytes_outside_the_ranges_are_zero():
    L = _L()
    for T, B, Cn, N, max_len in ((0, 2, 45, 3, 10), (40, 0, 45, 3, 10), (40, 65536, 45, 3, 10), (40, 2, 1, 3, 10), (40, 2, 257, 3, 10), (40, 2, 45, 0, 10),
                                 (40, 2, 45, 257, 10), (40, 2, 45, 3, -1), (40, 2, 45, 3, 256), (gc.tmax(45, 10) + 1, 2, 45, 3, 10)):
        assert L.mdd_ctc_nbest_grad_workspace_bytes(T, B, Cn, N, max_len) == 0, (T, B, Cn, N, max_len)


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_symbols_are_declared_listed_and_exported():
    from ctc_attention_mispronunciation_amd import _lib
    header = open(os.path.join(ROOT, "include", "mdd_hip.h")).read()
    for name in ("mdd_ctc_nbest_grad", "mdd_ctc_nbest_grad_fits", "mdd_ctc_nbest_grad_workspace_bytes", "mdd_nbest_risk"):
        assert re.search(r"\b(int|int64_t) %s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
    assert _lib.lib().mdd_version() == 100


def _grad_args(**over):
    a = dict(logp=_FAKE, T=40, B=3, C=45, len=_FAKE, ids=_FAKE, pitch=40, nids=_FAKE, N=10, max_len=10, blank=0, coef=_FAKE, loglik=None, grad=_FAKE,
             flag=_FAKE, ws=None, ws_bytes=0)
    a.update(over)
    vp = C.c_void_p
    return (vp(a["logp"]), a["T"], a["B"], a["C"], vp(a["len"]), vp(a["ids"]), a["pitch"], vp(a["nids"]), a["N"], a["max_len"], a["blank"],
            vp(a["coef"]), vp(a["loglik"]), vp(a["grad"]), vp(a["flag"]), vp(a["ws"]), a["ws_bytes"], None)


_GRAD_REFUSALS = [
    (dict(logp=None), "logp_dev"), (dict(len=None), "len_dev"), (dict(ids=None), "ids_dev"), (dict(nids=None), "nids_dev"), (dict(coef=None), "coef_dev"),
    (dict(grad=None), "grad_dev"), (dict(flag=None), "flag_dev"),
    (dict(N=0), "N<=256"), (dict(N=257), "N<=256"), (dict(B=0), "<=B"), (dict(B=65536), "B<=65535"), (dict(C=1), "C<=256"), (dict(C=257), "C<=256"),
    (dict(T=0), "T < 1"), (dict(blank=-1), "blank"), (dict(blank=45), "blank"),
    (dict(max_len=-1), "max_len"), (dict(max_len=256, pitch=300), "max_len"), (dict(max_len=41, pitch=40), "max_len"),
    (dict(T=20000), "T too long"), (dict(T=100, C=256, blank=0), "T too long"),
]


@pytest.mark.parametrize("over,needle", _GRAD_REFUSALS, ids=["_".join("%s=%s" % kv for kv in o.items()) for o, _ in _GRAD_REFUSALS])
def test_grad_entry_refuses_bad_arguments_on_the_host(over, needle):
    L = _L()
    assert L.mdd_ctc_nbest_grad(*_grad_args(**over)) == MDD_ERR_ARG
    msg = L.mdd_last_error().decode()
    assert msg.startswith("mdd_ctc_nbest_grad") and needle in msg, msg


def test_grad_entry_refuses_a_short_workspace_on_the_host():
    L = _L()
    need = gc.plan(40, 3, 45, 10, 10).bytes
    assert L.mdd_ctc_nbest_grad(*_grad_args(ws=_FAKE, ws_bytes=need - 1)) == MDD_ERR_ARG
    msg = L.mdd_last_error().decode()
    assert msg.startswith("mdd_ctc_nbest_grad") and "workspace_bytes" in msg and str(need) in msg, msg
    T = gc.tmax(45, 10)
    assert L.mdd_ctc_nbest_grad(*_grad_args(T=T + 1)) == MDD_ERR_ARG and "LDS" in L.mdd_last_error().decode()


_RISK_REFUSALS = [(dict(loglik=None), "loglik_dev"), (dict(cost=None), "cost_dev"), (dict(post=None), "post_dev"), (dict(risk=None), "risk_dev"),
                  (dict(coef=None), "coef_dev"), (dict(flag=None), "flag_dev"), (dict(N=0), "N<=256"), (dict(N=257), "N<=256"), (dict(B=0), "B < 1")]


@pytest.mark.parametrize("over,needle", _RISK_REFUSALS, ids=["_".join("%s=%s" % kv for kv in o.items()) for o, _ in _RISK_REFUSALS])
def test_risk_entry_refuses_bad_arguments_on_the_host(over, needle):
    a = dict(loglik=_FAKE, cost=_FAKE, status=None, N=5, B=3, post=_FAKE, risk=_FAKE, coef=_FAKE, flag=_FAKE)
    a.update(over)
    vp = C.c_void_p
    L = _L()
    assert L.mdd_nbest_risk(vp(a["loglik"]), vp(a["cost"]), vp(a["status"]), a["N"], a["B"], vp(a["post"]), vp(a["risk"]), vp(a["coef"]), vp(a["flag"]),
                            None) == MDD_ERR_ARG
    msg = L.mdd_last_error().decode()
    assert msg.startswith("mdd_nbest_risk") and needle in msg, msg


# ---------------------------------------------------------------------------------------------------------------- the conf
def _conf(tmp_path, **over):
    """A conf whose data files exist (empty: the checks under test come before any is read)."""
    conf = {}
    for k in ("train_wav_scp", "valid_wav_scp", "train_lab_path", "train_trans_path", "valid_lab_path", "valid_trans_path", "vocab_file"):
        path = tmp_path / k
        path.write_text("")
        conf[k] = str(path)
    conf["cmvn_path"] = str(tmp_path / "cmvn")
    conf["lm_path"] = os.path.join(GOLD, "lm_synth45.arpa")
    conf.update(over)
    return {k: v for k, v in conf.items() if v is not None}


@pytest.mark.parametrize("over,needle", [
    (dict(mwer_nbest=3, lm_path=None), "mwer_nbest needs lm_path"),
    (dict(mwer_nbest=12, mwer_beam_width=10), "mwer_nbest 12 exceeds mwer_beam_width 10"),
    (dict(mwer_nbest=1), "mwer_nbest 1: the N-best list of the MWER loss takes 2..256"),
    (dict(mwer_nbest=257), "mwer_nbest 257: the N-best list of the MWER loss takes 2..256"),
    (dict(init_model="/nonexistent/ctc_best_model.pkl"), "init_model: no file at /nonexistent/ctc_best_model.pkl"),
    (dict(mwer_nbest=3, init_model="/nonexistent/ctc_best_model.pkl"), "init_model: no file at"),
], ids=["no_lm_path", "n_above_beam", "n_1", "n_257", "init_model_missing", "init_model_missing_with_mwer"])
def test_conf_refusals(tmp_path, capsys, monkeypatch, over, needle):
    from ctc_attention_mispronunciation_amd.steps import train_ctc
    import torch
    monkeypatch.setattr(torch, "manual_seed", lambda *a: pytest.fail("the conf was not refused before the seeds"))
    with pytest.raises(SystemExit) as e:
        train_ctc.main(_conf(tmp_path, **over))
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert needle in err and len(err.strip().splitlines()) == 1, err


def test_conf_defaults(tmp_path):
    from ctc_attention_mispronunciation_amd.steps import train_ctc
    assert train_ctc.check_mwer(_conf(tmp_path)) == (0, 0) and train_ctc.check_mwer(_conf(tmp_path, mwer_nbest=0)) == (0, 0)
    assert train_ctc.check_mwer(_conf(tmp_path, mwer_nbest=3)) == (3, 10) and train_ctc.check_mwer(_conf(tmp_path, mwer_nbest=40)) == (40, 40)
    assert train_ctc.check_mwer(_conf(tmp_path, mwer_nbest=256)) == (256, 256) and train_ctc.check_mwer(_conf(tmp_path, mwer_nbest=5, mwer_beam_width=64)) == (5, 64)
