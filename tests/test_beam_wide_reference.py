"""The host side of mdd_beam_wide / mdd_beam_fits / mdd_beam_wide_workspace_bytes and the yardsticks of tests/test_beam_wide.py, without a GPU.

  * G17 (tools/gen_golden_beam_wide.py: the reference's own BeamDecoder with its default constructor arguments -- beam 200, lm_alpha 0.01 --
    and at beam 100 / alpha 0.25): oracle.beam's winners are the reference's strings and the Python N-best yardstick's lists are the
    reference's final lists, so both yardsticks are tied to the reference at the widths only the wide entry takes;
  * the cases of the GPU half (WIDE_CASES, LONG_CASES, TIE_CASES, ...) are robust by the rules of tests/test_decoders.py and
    tests/test_nbest_reference.py: the oracle and the Python port agree, every row that is not meant to fail has status 0, and where
    whole lists are compared they rank alike under both exp flavours with neighbouring scores equal or more than 2 SCORE_RTOL apart;
  * the three symbols; every refusal of mdd_beam_wide (fake pointers: none of them reaches a device call); mdd_beam_fits against
    beam_accepts over a grid; mdd_beam_wide_workspace_bytes against the sum written out below.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import nbest_reference as nr
from tests.helpers import GOLD, ROOT, jload, npz
from tests.test_decoders import (ERROR_ROWS, KB, MDD_ERR_ARG, SCORE_RTOL, Case, _FAKE, _L, _check_robust, beam_accepts, expected, fast_eligible,
                                 generic_lds_bytes, inputs)
from tests.test_nbest_reference import _check_case

WIDE_BEAM_MAX, WIDE_T_MAX = 256, 38400


def _lens(T):
    """B = 3 utterances of T, 5 T / 6 and T / 2 - 3 frames, and one of length 0, which must come out as status 1 (IndexError)."""
    return (T, T * 5 // 6, T // 2 - 3, 0)


def _wide(beam, Cn, T, alpha, blank=0, family="flat", seed=0):
    name = "wide_%s_b%d_C%d_T%d_a%g_blank%d" % (family, beam, Cn, T, alpha, blank)
    return Case(name, family, Cn, beam, blank, alpha, T, 4, seed or 1000 + beam + Cn + T + blank, lens=_lens(T))


# 2. shapes only the wide entry accepts: beam > 64, or beam * C past the generic kernel's LDS
WIDE_CASES = [_wide(65, 45, 40, 0.01), _wide(65, 45, 40, 0.25), _wide(200, 45, 40, 0.01), _wide(200, 45, 40, 0.25),
              _wide(200, 45, 40, 0.01, family="peaky"), _wide(256, 9, 30, 0.2), _wide(64, 256, 30, 0.2), _wide(100, 100, 30, 0.2),
              _wide(65, 45, 40, 0.2, blank=22), _wide(65, 45, 40, 0.2, blank=44)]
# 3. past the T limits of the LDS kernels (663 at beam 64, 3995 at beam 10), peaky, one utterance
LONG_CASES = [Case("long_b%d_C45_T%d" % (beam, T), "peaky", 45, beam, 0, 0.0, T, 1, 700 + beam) for beam, T in ((64, 664), (10, 3996), (20, 3500))]
# 4. shapes both entries accept: (10, 45) the single-wave kernel, (16, 64) its 16-slot form, (17, 45) and (64, 45) the generic kernel
BOTH_SHAPES = ((10, 45, 60), (16, 64, 40), (17, 45, 40), (64, 45, 40))
BOTH_CASES = [Case("both_%s_b%d_C%d_T%d" % (fam, beam, Cn, T), fam, Cn, beam, 0, 0.0 if fam in ("tied", "uniform") else 0.2, T,
                   12 if fam == "errors" else 3, 800 + beam + Cn, lens=None if fam == "errors" else (T, T * 5 // 6, T // 2 - 3))
              for beam, Cn, T in BOTH_SHAPES for fam in ("flat", "tied", "uniform", "errors")]
# 5. exact ties past 64 beams (beam * C <= 4500: on a full tie the rank count is quadratic in it)
TIE_CASES = [Case("wtie_%s_b%d_C%d" % (fam, beam, Cn), fam, Cn, beam, 0, 0.0, 20, 2, 900 + beam + Cn, lens=(20, 13))
             for fam in ("tied", "uniform") for beam, Cn in ((100, 45), (65, 12))]
# 6. the first error, 7. the whole list at the reference's default width, 9. more utterances than CUs
ERROR_CASE = Case("werrors_b100_C45", "errors", 45, 100, 0, 0.2, 24, 12, 951)
NBEST_CASE = Case("wnbest_b200_C45_T30", "flat", 45, 200, 0, 0.01, 30, 2, 961, lens=(30, 23))
MANY_CASE = Case("wmany_b65_C45_B257", "flat", 45, 65, 0, 0.2, 24, 257, 971, ragged=True, port_rows=12)
ALL_CASES = WIDE_CASES + LONG_CASES + BOTH_CASES + TIE_CASES + [ERROR_CASE, NBEST_CASE, MANY_CASE]
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


# ------------------------------------------------------------------------------------------------------------------ G17
G17_STATUS0 = "every G17 utterance decodes"


def g17():
    meta, g = jload("g17_beam_wide.json"), npz("g17_beam_wide.npz")
    assert meta["C"] == 45 and meta["T"] == 40 and meta["lens"] == [40, 33, 17, 26] and meta["blank"] == 0
    assert meta["settings"] == {"default": {"beam": 200, "alpha": 0.01}, "b100": {"beam": 100, "alpha": 0.25}}
    return meta, g


def g17_lists(g, setting, kind, b):
    ids, scores = g["%s_%s_u%d_ids" % (setting, kind, b)], g["%s_%s_u%d_scores" % (setting, kind, b)]
    return [[int(k) for k in row if k >= 0] for row in ids], scores


@pytest.mark.parametrize("kind", ["peaky", "flat"])
@pytest.mark.parametrize("setting", ["default", "b100"])
def test_yardsticks_reproduce_the_reference_at_wide_beams(setting, kind):
    from ctc_attention_mispronunciation_amd import synth
    meta, g = g17()
    i2c = synth.phone_table_41()
    beam, alpha = meta["settings"][setting]["beam"], meta["settings"][setting]["alpha"]
    logp, lens, table = g[kind], g["lens"], g["lm45"]
    assert logp.shape == (40, 4, 45) and logp.dtype == np.float32
    want, st, sc = oracle.beam(logp, lens, table, beam_width=beam, alpha=alpha, blank=0, return_scores=True)
    assert (st == 0).all(), G17_STATUS0
    assert [" ".join(i2c[k] for k in w) for w in want] == meta["batches"][kind]["best"][setting]
    for flavour in nr.EXP_FLAVOURS:
        for b, (final, status) in enumerate(nr.nbest(logp, lens, table, beam, alpha, 0, flavour)):
            ids, scores = g17_lists(g, setting, kind, b)
            assert status == 0 and len(final) == beam == len(ids)
            assert [y for y, _ in final] == ids, (flavour, b)
            assert ids[0] == want[b]
            if flavour == "torch":
                np.testing.assert_allclose([s for _, s in final], scores, rtol=1e-12, atol=0)
                assert abs(scores[0] - sc[b]) <= SCORE_RTOL * abs(sc[b])
    for b in range(4):                                       # the lists are robust: a GPU list within SCORE_RTOL ranks the same way
        _, scores = g17_lists(g, setting, kind, b)
        for s0, s1 in zip(scores, scores[1:]):
            assert s0 == s1 or (s0 - s1) > 2 * SCORE_RTOL * max(abs(s0), abs(s1)), (b, s0, s1)


# ----------------------------------------------------------------------------------------- the cases of the GPU half are robust
def _ok_rows(case):
    """status the yardstick must report: 0 on every row that is not meant to fail."""
    _, lens, _ = inputs(case)
    if case.family == "errors":
        return [ERROR_ROWS[b % len(ERROR_ROWS)][1] for b in range(case.B)]
    return [0 if min(int(n), case.T) > 0 else 1 for n in lens]


@pytest.mark.parametrize("name", [c.name for c in WIDE_CASES + LONG_CASES + [MANY_CASE]])
def test_oracle_and_python_port_agree_on_the_wide_cases(name):
    case = BY_NAME[name]
    _check_robust(case)
    _, st, _ = expected(case)
    if case is MANY_CASE:                      # ragged: row 1 has no frame and row 2 one, after which the state's 45 entries -- fewer than the
        _, lens, _ = inputs(case)              # beam -- still hold the empty prefix: IndexError, as in a row of two frames that keeps it; the rest decodes
        assert st[1] == st[2] == 1 and set(st.tolist()) == {0, 1} and (lens[st != 0] <= 2).all() and (st != 0).sum() <= 4
    else:
        assert st.tolist() == _ok_rows(case), name
    assert not beam_accepts(case.beam, case.C, case.T) or case.beam > 64


def test_error_rows_at_a_wide_beam():
    """The `errors` family at beam 100.  Its rows are built for narrow beams (p1 and p2 lie 40 nats down, so that only the row that lifts
    them keeps them): with 100 beams the first frame keeps all 44 extensions, the p1 beam among them, so the rows that were clean meet
    the KeyError on the second frame.  The order of the first error still decides: row 4 (a zero posterior at rank 0, the NaN of the LM in
    a lower beam) is a ValueError among KeyErrors, and rows 7 and 8 (nothing but blanks, no frames) end in IndexError; the oracle and the
    Python port agree on every row."""
    from tests.test_decoders import _port_beam
    want, st, _ = expected(ERROR_CASE)
    ids, status = _port_beam(ERROR_CASE, ERROR_CASE.B)
    assert status == st.tolist() == [3, 3, 3, 3, 2, 3, 3, 1, 1, 3, 3, 3] and ids == want
    assert [ERROR_ROWS[b][0] for b in (4, 7, 8)] == ["value_rank0_key_lower", "all_blank", "len0"]


def test_spread_rows_of_the_many_utterance_case_are_robust():
    """The GPU half compares the rows nbest_reference.spread_rows picks: on each the winner is the oracle's under both exp flavours."""
    want, st, _ = expected(MANY_CASE)
    rows, lists = nr.case_lists(MANY_CASE, "torch")
    _, lists64 = nr.case_lists(MANY_CASE, "f64")
    assert len(rows) >= 12 and rows[-1] == MANY_CASE.B - 1
    for b, (final, status), (final64, status64) in zip(rows, lists, lists64):
        assert status == status64 == st[b] == 0, b
        assert final[0][0] == final64[0][0] == want[b], b


@pytest.mark.parametrize("name", [c.name for c in TIE_CASES + [NBEST_CASE]])
def test_yardstick_lists_of_the_wide_cases_are_robust(name):
    case = BY_NAME[name]
    tie = _check_case(case)
    _, st, _ = expected(case)
    assert (st == 0).all()
    if case in TIE_CASES:
        assert tie, "a tie case without an exact tie inside its final list"
        assert case.beam * case.C <= 4500


@pytest.mark.parametrize("name", [c.name for c in BOTH_CASES])
def test_both_entry_cases_are_accepted_by_both(name):
    case = BY_NAME[name]
    assert beam_accepts(case.beam, case.C, case.T)
    _, st, _ = expected(case)
    if case.family == "errors":                              # (beam 64 keeps every class of the first frame: see test_error_rows_at_a_wide_beam)
        assert st.tolist() == (_ok_rows(case) if case.beam < 45 else [3, 3, 3, 3, 2, 3, 3, 1, 1, 3, 3, 3])
    else:
        assert (st == 0).all()
    assert fast_eligible(case.beam, case.C) == ((case.beam, case.C) in ((10, 45), (16, 64)))


# --------------------------------------------------------------------------------------------------------------- symbols
def test_symbols_are_declared_listed_and_exported():
    from ctc_attention_mispronunciation_amd import _lib
    header = open(os.path.join(ROOT, "include", "mdd_hip.h")).read()
    assert re.search(r"\bint32_t mdd_beam_fits\s*\(", header)
    assert re.search(r"\bint64_t mdd_beam_wide_workspace_bytes\s*\(", header)
    assert re.search(r"\bint mdd_beam_wide\s*\(", header)
    for name in ("mdd_beam_fits", "mdd_beam_wide_workspace_bytes", "mdd_beam_wide"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
    assert _lib.lib().mdd_version() == 100


# -------------------------------------------------------------------------------------------------------------- refusals
def wide_args(**over):
    a = dict(logp=_FAKE, T=10, B=2, C=45, len=_FAKE, beam=100, blank=0, lm=_FAKE, alpha=0.0, nbest=None, ids=_FAKE, nids=_FAKE, status=_FAKE,
             score=_FAKE, ws=None, ws_bytes=0)
    a.update(over)
    nbest = a["beam"] if a["nbest"] is None else a["nbest"]
    return (C.c_void_p(a["logp"]), a["T"], a["B"], a["C"], C.c_void_p(a["len"]), a["beam"], a["blank"], C.c_void_p(a["lm"]),
            C.c_double(a["alpha"]), nbest, C.c_void_p(a["ids"]), C.c_void_p(a["nids"]), C.c_void_p(a["status"]), C.c_void_p(a["score"]),
            C.c_void_p(a["ws"]), C.c_int64(a["ws_bytes"]), None)


@pytest.mark.parametrize("over", [dict(beam=0, nbest=1), dict(beam=257, nbest=1), dict(C=1), dict(C=257), dict(blank=-1), dict(blank=45),
                                  dict(T=0), dict(T=WIDE_T_MAX + 1), dict(B=0), dict(nbest=0), dict(nbest=101), dict(logp=None),
                                  dict(len=None), dict(lm=None), dict(ids=None), dict(nids=None), dict(status=None), dict(score=None)],
                         ids=lambda o: "_".join("%s=%s" % kv for kv in o.items()))
def test_wide_bad_arguments_are_refused_on_the_host(over):
    """None of these reaches a device call (this test runs without a GPU)."""
    L = _L()
    assert L.mdd_beam_wide(*wide_args(**over)) == MDD_ERR_ARG
    msg = L.mdd_last_error().decode()
    assert msg.startswith("mdd_beam_wide"), msg
    if "nbest" in over and "beam" not in over:
        assert "nbest" in msg, msg


def test_wide_refuses_a_workspace_one_byte_short():
    L = _L()
    need = L.mdd_beam_wide_workspace_bytes(10, 2, 45, 100)
    assert need > 0
    assert L.mdd_beam_wide(*wide_args(ws=_FAKE, ws_bytes=need - 1)) == MDD_ERR_ARG
    msg = L.mdd_last_error().decode()
    assert msg.startswith("mdd_beam_wide") and "mdd_beam_wide_workspace_bytes" in msg and str(need) in msg, msg


# --------------------------------------------------------------------------------------------------------- mdd_beam_fits
def _max_T(beam, Cn):
    """The largest T mdd_beam accepts at (beam, C), 0 when it accepts none (acceptance falls with T: both LDS sums grow with it, and the
    one step down -- the LM table leaving LDS -- happens below the 140 KB bound)."""
    if not beam_accepts(beam, Cn, 1):
        return 0
    lo, hi = 1, 1 << 20
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if beam_accepts(beam, Cn, mid) else (lo, mid)
    return lo


def test_fits_is_the_beam_entries_acceptance(monkeypatch):
    for var in ("MDD_BEAM_GENERIC", "MDD_BEAM_W"):
        monkeypatch.delenv(var, raising=False)
    fits = _L().mdd_beam_fits
    checked = refused = 0
    for Cn in (2, 9, 45, 64, 65, 100, 256):
        for beam in range(1, 65):
            top = _max_T(beam, Cn)
            for T in sorted({1, 30, 664, 3500} | {t for t in range(top - 8, top + 10) if t >= 1}):
                want = beam_accepts(beam, Cn, T)
                assert fits(T, 3, Cn, beam) == int(want), (beam, Cn, T)
                checked += 1
                refused += not want
    assert checked > 7000 and refused > 3000
    assert _max_T(10, 45) == 3995 and _max_T(64, 45) == 663 and _max_T(64, 256) == 0
    for T, B, Cn, beam in ((10, 2, 45, 65), (10, 2, 45, 200), (10, 2, 257, 10), (10, 2, 1, 10), (0, 2, 45, 10), (10, 0, 45, 10), (10, 2, 45, 0),
                           (-1, 2, 45, 10)):
        assert fits(T, B, Cn, beam) == 0, (T, B, Cn, beam)
    assert fits(38401, 1, 45, 1) == int(beam_accepts(1, 45, 38401))      # no bound on T but the LDS sums
    # the switches as mdd_beam reads them: under MDD_BEAM_GENERIC the single-wave kernel's limit does not apply
    assert fits(4000, 1, 45, 10) == 0 and generic_lds_bytes(10, 45, 4000) <= 140 * KB
    monkeypatch.setenv("MDD_BEAM_GENERIC", "1")
    assert fits(4000, 1, 45, 10) == 1 and fits(6500, 1, 45, 10) == int(generic_lds_bytes(10, 45, 6500) <= 140 * KB) == 0


# ------------------------------------------------------------------------------------------ mdd_beam_wide_workspace_bytes
LDS_BUDGET = 112 * KB      # csrc/plan.h: kBeamWideLdsBudget, the wide kernel's dynamic LDS


def _r16(v):
    return (v + 15) & ~15


def workspace_bytes(T, B, Cn, beam):
    """csrc/plan.h, beam_wide_plan, written out: the pre-pass's fp64 log-probs and flags; per utterance the live-frame list, two sets of
    `beam` prefix rows of Tcap bytes, the candidate totals where 8 beam C is over the LDS budget, and a full-size compacted list (fp64
    value + int order) where what the totals leave of the budget holds fewer than beam C entries of 12 bytes.  Every part is rounded up
    to 16 bytes."""
    n, tcap = beam * Cn, (T + 4) & ~3
    tot_lds = 8 * n if 8 * n <= LDS_BUDGET else 0
    cap = min(((LDS_BUDGET - tot_lds) // 12) & ~1, n)
    utt = _r16(4 * T) + _r16(2 * beam * tcap)
    if not tot_lds:
        utt += _r16(8 * n)
    if cap < n:
        utt += _r16(8 * n) + _r16(4 * n)
    return _r16(8 * T * B * Cn) + _r16(T * B) + B * utt


def test_workspace_bytes_is_the_stated_sum():
    f = _L().mdd_beam_wide_workspace_bytes
    shapes = [(T, B, Cn, beam) for T in (1, 2, 3, 4, 5, 39, 40, 664, 3500, WIDE_T_MAX) for B in (1, 3, 64, 257) for Cn in (2, 9, 45, 100, 256)
              for beam in (1, 10, 64, 65, 100, 200, 255, 256)]
    for T, B, Cn, beam in shapes:
        got = f(T, B, Cn, beam)
        assert got == workspace_bytes(T, B, Cn, beam) and got > 0 and got % 16 == 0, (T, B, Cn, beam)
    # the placements the restatement distinguishes all occur: everything in LDS, the list's overflow in the workspace, the totals too
    assert 20 * 65 * 45 <= LDS_BUDGET < 20 * 200 * 45 and 8 * 200 * 45 <= LDS_BUDGET < 8 * 64 * 256
    assert f(40, 1, 45, 200) - f(40, 1, 45, 65) > 12 * 200 * 45 and f(30, 1, 256, 64) - f(30, 1, 255, 64) > 0
    # non-decreasing in each of T, B and beam
    for T, B, Cn, beam in shapes:
        base = f(T, B, Cn, beam)
        if T < WIDE_T_MAX:
            assert f(T + 1, B, Cn, beam) >= base
        assert f(T, B + 1, Cn, beam) >= base
        if beam < WIDE_BEAM_MAX:
            assert f(T, B, Cn, beam + 1) >= base, (T, B, Cn, beam)
    for T, B, Cn, beam in ((0, 1, 45, 10), (WIDE_T_MAX + 1, 1, 45, 10), (10, 0, 45, 10), (10, 1, 1, 10), (10, 1, 257, 10), (10, 1, 45, 0), (10, 1, 45, 257)):
        assert f(T, B, Cn, beam) == 0
    assert f(WIDE_T_MAX, 1024, 256, 256) > 1 << 32       # a 64-bit count
