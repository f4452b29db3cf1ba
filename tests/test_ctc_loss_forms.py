"""``mdd_ctc_loss`` (csrc/ctc.hip) against float64 on both sides of every place its scan changes form: the wave kernel at 1, 2 and 4 labels
per lane and the generic kernel in its own regime (Lmax >= 256, C > 256, log-probs past the wave form's 128 KB of LDS), peaked inputs, the
blank at the first, a middle and the last class, rows without labels, clamped input lengths, a row that a single path satisfies.  The cases
and the reference are tests/ctc_loss_cases.py's (CPU ``torch.nn.functional.ctc_loss`` on a double tensor); every wave-form case runs a second
time with the generic kernel forced (``MDD_CTC=generic``).

Bounds, per kernel form (``ctc_loss_cases.bounds``): the larger of the project's present bound -- nll rtol 1e-6, gradient atol 5e-6 (wave) and
2e-6 (generic) -- and twice the worst value tools/ctc_loss_margins.py measured on an MI355X over every run of the table in that form
(profiles/ctc_loss_margins.json).  Beside it, per case, the kernel's gradient error may not exceed that of ATen's fp32 run of the same
input: this path is meant to be closer to float64 than ATen's fp32.

Per run also: padded frames exactly 0; |sum over classes| of every frame's gradient <= 1e-4; a second run, a run with a caller workspace of
exactly ``mdd_ctc_workspace_bytes`` and (for the nll) a run without gradient give the same bits; a workspace one double short is refused
with MDD_ERR_ARG before any device work -- a size that disagreed with the launch at a form boundary would overrun or be refused here."""
import ctypes as C

import numpy as np
import pytest

from tests import ctc_loss_cases as cc

MDD_ERR_ARG = -1
pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def run_library(c, want_grad=True):
    """hip_model.ctc_loss: the workspace comes from the binding."""
    import torch
    from ctc_attention_mispronunciation_amd.hip_model import ctc_loss
    return ctc_loss(torch.from_numpy(np.array(c.lp)).cuda(), torch.from_numpy(np.array(c.tg)), torch.from_numpy(np.array(c.il)),
                    torch.from_numpy(np.array(c.tl)), blank=c.blank, want_grad=want_grad)


def run_caller_workspace(c, short=0):
    """mdd_ctc_loss through ctypes with a caller workspace of mdd_ctc_workspace_bytes - short bytes; the outputs start as NaN, so whatever
    the kernel leaves unwritten shows.  Returns (status, nll, grad)."""
    import torch
    from ctc_attention_mispronunciation_amd import _lib
    L_ = _lib.lib()
    T, B, Cn = c.lp.shape
    L = c.tg.shape[1]
    d = lambda a: torch.from_numpy(np.array(a)).cuda()      # noqa: E731
    lp, tg, il, tl = d(c.lp), d(c.tg), d(c.il), d(c.tl)
    nll = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda")
    grad = torch.full((T, B, Cn), float("nan"), dtype=torch.float32, device="cuda")
    need = L_.mdd_ctc_workspace_bytes(T, B, Cn, L, 1)
    assert need == (8 * B * T * (2 * L + 1) if _form_now(c) == "generic" else 16 * B * T * 2 * (L + 1))
    ws = torch.zeros((need - short) // 8, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    rc = L_.mdd_ctc_loss(p(lp), T, B, Cn, p(tg), L, p(il), p(tl), c.blank, p(nll), p(grad), p(ws), ws.numel() * 8, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, nll, grad


def _form_now(c):
    import os
    return "generic" if os.environ.get("MDD_CTC") == "generic" else c.form


def measure(name):
    """One run of a case through whichever kernel the library routes it to now: its errors against the float64 reference, and the outputs."""
    c = cc.case(name)
    ref_nll, ref_grad = cc.reference(name)
    nll, grad = run_library(c)
    return dict(nll_rel_err=cc.nll_rel_err(nll.cpu().numpy(), ref_nll), grad_abs_err=cc.grad_abs_err(grad.cpu().numpy(), ref_grad)), nll, grad


@pytest.mark.parametrize("name,form,forced", cc.runs(), ids=[cc.run_id(*r) for r in cc.runs()])
def test_ctc_loss_against_float64(name, form, forced, monkeypatch):
    if forced:
        monkeypatch.setenv("MDD_CTC", "generic")
    else:
        monkeypatch.delenv("MDD_CTC", raising=False)
    c = cc.case(name)
    T, B, Cn = c.lp.shape
    assert _form_now(c) == form
    err, nll, grad = measure(name)
    rtol, atol = cc.bounds(form)
    aten_nll, aten_grad = cc.aten_err(name)
    print("%s: nll rel %.3e (bound %.1e, ATen fp32 %.2e)  grad abs %.3e (bound %.1e, ATen fp32 %.2e)"
          % (cc.run_id(name, form, forced), err["nll_rel_err"], rtol, aten_nll, err["grad_abs_err"], atol, aten_grad))
    assert err["nll_rel_err"] <= rtol
    assert err["grad_abs_err"] <= atol
    assert err["grad_abs_err"] <= aten_grad, "farther from float64 than ATen's fp32"
    g = grad.cpu().numpy()
    for b in range(B):
        assert not g[c.il_ref[b]:, b].any(), "row %d: a padded frame carries gradient" % b
    assert np.abs(g.astype(np.float64).sum(-1)).max() <= cc.CLASS_SUM
    if c.spec.kind == "clamp":
        assert np.isposinf(nll.cpu().numpy()[1]) and not g[:, 1].any()      # clamped to no frames, with labels to emit
    # the same bits: a second run, the nll alone, a caller workspace of exactly the stated size
    nll2, grad2 = run_library(c)
    assert (_bits(nll2) == _bits(nll)).all() and (_bits(grad2) == _bits(grad)).all()
    nll3, none = run_library(c, want_grad=False)
    assert none is None and (_bits(nll3) == _bits(nll)).all()
    rc, nll4, grad4 = run_caller_workspace(c)
    assert rc == 0
    assert (_bits(nll4) == _bits(nll)).all() and (_bits(grad4) == _bits(grad)).all()
    # one double short: refused, nothing written
    from ctc_attention_mispronunciation_amd import _lib
    rc, nll5, grad5 = run_caller_workspace(c, short=8)
    assert rc == MDD_ERR_ARG and "workspace" in _lib.lib().mdd_last_error().decode()
    assert bool(nll5.isnan().all()) and bool(grad5.isnan().all())
