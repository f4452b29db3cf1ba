"""CPU side of tests/ctc_loss_cases.py: the form rule against the library's own workspace size (host-only, no GPU), the boundaries the
neighbouring cases straddle, the conditions on the inputs that make the float64 reference a reference, and ATen's fp32 distance from it, the
figure the GPU test holds the kernels beside."""
import numpy as np
import pytest

from tests import ctc_loss_cases as cc


def _lib():
    from ctc_attention_mispronunciation_amd import _lib
    return _lib.lib()


def test_table_reaches_what_it_names():
    form = {n: cc.case(n).form for n in cc.NAMES}
    assert form["lds45_T712"] == "wave1" and form["lds45_T713"] == "generic"
    assert cc.T101 == 317 and form["lds101_T317"] == "wave1" and form["lds101_T318"] == "generic"
    assert form["lane_L127"] == "wave2" and form["lane_L128"] == "wave4" and form["form_L255"] == "wave4"
    for n in ("form_L256", "long_L300", "wide_C257_blank256", "wide_C300"):
        assert form[n] == "generic", n
    for n in ("peaked_x30", "peaked_x12_blank44", "blank22", "repeats_T81", "repeats_T79", "clamp", "ends_blank0", "ends_blank6"):
        assert form[n] == "wave1", n
    for a, b in cc.PAIRS:
        sa, sb = cc.SPECS[a], cc.SPECS[b]
        assert form[a] != form[b] and form[a] != "generic", (a, b)
        assert (sa.C, sa.blank) == (sb.C, sb.blank) and abs(sa.T - sb.T) <= 1 and abs(sa.L - sb.L) <= 1      # neighbours: one step apart
    # every peaked case and every blank position also runs through the generic kernel
    forced = {n for n, f, forced in cc.runs() if forced}
    assert {"peaked_x30", "peaked_x12_blank44", "blank22", "ends_blank6"} <= forced
    assert {cc.SPECS[n].blank for n in cc.NAMES} >= {0, 6, 22, 44, 256}
    assert set(f for _, f, _ in cc.runs()) == set(cc.FORMS)


@pytest.mark.parametrize("name", cc.NAMES)
def test_expected_form_agrees_with_the_library_workspace(name):
    """mdd_ctc_workspace_bytes switches size where expected_form says the launch switches kernels: 16 B T 2 (Lmax + 1) bytes of alpha and
    beta rows for the wave form, 8 B T (2 Lmax + 1) of alpha rows for the generic one, nothing without a gradient."""
    c = cc.case(name)
    T, B, C = c.lp.shape
    L = c.tg.shape[1]
    L_ = _lib()
    wave, generic = 16 * B * T * 2 * (L + 1), 8 * B * T * (2 * L + 1)
    assert wave != generic
    assert L_.mdd_ctc_workspace_bytes(T, B, C, L, 1) == (generic if c.form == "generic" else wave) == cc.expected_workspace_bytes(T, B, C, L)
    assert L_.mdd_ctc_workspace_bytes(T, B, C, L, 0) == 0


def test_lds_rule_over_a_sweep_of_shapes():
    """Beyond the table: the rule and the library agree on every T around each switch, at every labels-per-lane width."""
    L_ = _lib()
    for C, L in ((45, 40), (45, 100), (45, 200), (101, 20), (101, 127), (256, 63), (256, 255), (7, 5)):
        last = cc.last_wave_T(C, L)
        for T in (1, last - 1, last, last + 1, last + 2, 2 * last):
            assert L_.mdd_ctc_workspace_bytes(T, 2, C, L, 1) == cc.expected_workspace_bytes(T, 2, C, L), (T, C, L)
    for C, L in ((257, 12), (300, 12), (45, 256), (45, 300)):
        assert cc.expected_form(8, C, L) == "generic" and L_.mdd_ctc_workspace_bytes(8, 2, C, L, 1) == 8 * 2 * 8 * (2 * L + 1)


@pytest.mark.parametrize("name", cc.NAMES)
def test_inputs_and_reference(name, capsys):
    c = cc.case(name)
    T, B, C = c.lp.shape
    s = c.spec
    assert (T, C, c.tg.shape[1], c.blank) == (s.T, s.C, s.L, s.blank)
    assert c.lp.dtype == np.float32 and np.isfinite(c.lp).all() and abs(np.exp(c.lp.astype(np.float64)).sum(-1) - 1.0).max() < 1e-5
    assert c.tl[0] == s.L and c.il_ref[0] == T                      # row 0: full lengths
    assert ((c.tg >= 0) & (c.tg < C) & (c.tg != c.blank)).all()
    assert (c.il_ref == np.clip(c.il, 0, T)).all()
    nll, grad = cc.reference(name)
    assert nll.dtype == np.float64 and grad.dtype == np.float64 and grad.shape == c.lp.shape
    finite = np.ones(B, dtype=bool)
    if s.kind == "clamp":
        assert c.il.tolist() == [T + 7, -2, T] and c.tl[1] > 0
        assert np.isposinf(nll[1]) and not grad[:, 1].any()         # no frames, some labels: +inf and a gradient of zero
        finite[1] = False
    assert np.isfinite(nll[finite]).all() and np.isfinite(grad).all(), nll
    for b in range(B):
        assert not grad[c.il_ref[b]:, b].any()
        if finite[b] and c.il_ref[b]:
            # the occupancies of a frame sum to 1, so the class sum is what the fp32 rounding of lp leaves of sum exp(lp) - 1
            excess = np.exp(c.lp[:c.il_ref[b], b].astype(np.float64)).sum(-1) - 1.0
            assert abs(grad[:c.il_ref[b], b].sum(-1) - excess).max() < 1e-9 and abs(excess).max() < 1e-5
        if c.tl[b] == 0:                                           # only blanks: nll = -sum_t lp[t, blank]
            want = -c.lp[:c.il_ref[b], b, c.blank].astype(np.float64).sum()
            assert abs(nll[b] - want) <= 1e-12 * abs(want), (b, nll[b], want)
    if s.kind != "ends":
        assert c.tl[2] == 0 and c.tl[1] < s.L and c.il_ref[1] < T
    if name == "repeats_T79":
        # one path: label, blank, label, ...; nll is the sum along it and the occupancies are 1 on it
        k = int(c.tg[0, 0])
        path = [k if t % 2 == 0 else c.blank for t in range(T)]
        want = -sum(float(c.lp[t, 0, path[t]]) for t in range(T))
        assert abs(nll[0] - want) <= 1e-12 * abs(want)
    if s.scale >= 12.0:
        assert c.lp.min() < (-180.0 if s.scale >= 30.0 else -60.0)
    # ATen's fp32 distance from the float64 reference, recorded per case: 7e-6 at T = 20 .. 9e-3 on peaked inputs
    n32, g32 = cc.aten_fp32(name)
    assert np.isfinite(n32[finite]).all() and np.isfinite(g32).all()
    e_nll, e_grad = cc.aten_err(name)
    with capsys.disabled():
        print("\n%-20s %-7s B %d  ATen fp32 against float64: nll rel %.2e  grad abs %.2e" % (name, c.form, B, e_nll, e_grad))
    assert 0.0 < e_grad < 5e-2 and e_nll < 1e-4


def test_margins_file_covers_every_run():
    """profiles/ctc_loss_margins.json holds one entry per run of the table, and the asserted bounds are never below the project's present ones."""
    m = cc.margins()
    assert set(m["runs"]) == {cc.run_id(*r) for r in cc.runs()}
    for name, form, forced in cc.runs():
        r = m["runs"][cc.run_id(name, form, forced)]
        assert r["form"] == form and r["case"] == name and np.isfinite([r["nll_rel_err"], r["grad_abs_err"], r["aten_grad_abs_err"]]).all()
    for form in cc.FORMS:
        rtol, atol = cc.bounds(form)
        assert cc.NLL_RTOL <= rtol < 1e-4 and cc.GRAD_ATOL[form] <= atol < 1e-3, (form, rtol, atol)
