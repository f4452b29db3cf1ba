"""The N-best yardstick (tests/nbest_reference.py) and the host side of mdd_beam_nbest, without a GPU.

  * the yardstick against G16 (the reference's own final sort, tools/gen_golden_nbest.py): identical ranked ids and statuses, scores
    within 1e-12 relative (the same float64 operations; only the libm may differ);
  * on every decoder case (tests/test_decoders.py: CASES and the two T-limit cases) its rank 0 and status are oracle.beam's winner and
    status, and a status-0 list has exactly `beam` entries (asserted inside the yardstick: the reason the ABI has no count output);
  * robustness, the rule of test_decoders extended to the list: the GPU rounds exp() differently from the reference, so a case must rank
    identically under both exp flavours and neighbouring scores must be exactly equal or more than 2 SCORE_RTOL apart; a case that is
    not gets another seed in RESEEDED below, never a skip or a tolerance;
  * the host refusals of mdd_beam_nbest, the symbol, nbest_posteriors, and the refusals of infer --nbest.
"""
import os
import re

import numpy as np
import pytest

from tests import nbest_reference as nr
from tests.helpers import GOLD, ROOT, jload, npz
from tests.test_decoders import (CASES, LIMIT_SHAPES, MDD_ERR_ARG, SCORE_RTOL, _beam_args, _L, beam_accepts, expected, limit_case,
                                 test_beam_bad_arguments_are_refused_on_the_host as _beam_refusals)

# case name -> seed, for the cases of CASES whose list is not robust under their own seed (two neighbouring scores closer than
# 2 SCORE_RTOL: a long utterance divides small differences by a long length).  Everything else of the case stays.
RESEEDED = {"generic_b64_C45_T200_a0_blank0": 5509, "long_T253_b10": 5563, "long_T300_b10": 2610, "long_T300_b20": 3620,
            "long_T520_b10": 7830, "long_T520_b16": 6836, "long_T520_b20": 17840, "long_T300_b16_C64_blank63": 20364}
NBEST_CASES = [c._replace(seed=RESEEDED[c.name]) if c.name in RESEEDED else c for c in CASES]
NBEST_BY_NAME = {c.name: c for c in NBEST_CASES}
LIMIT_CASES = {shape: limit_case(*shape) for shape in LIMIT_SHAPES}
TIE_FAMILIES = ("tied", "uniform", "mergetie")


# ------------------------------------------------------------------------------------------------------------------ G16
def test_yardstick_reproduces_the_reference_lists():
    meta, g = jload("g16_nbest.json"), npz("g16_nbest.npz")
    assert meta["C"] == 45 and {u["beam"] for u in meta["utterances"]} == {3, 10, 20} and {u["alpha"] for u in meta["utterances"]} == {0.0, 0.25}
    assert {u["error"] for u in meta["utterances"]} == {None, "IndexError", "ValueError", "KeyError"}
    tied = 0
    for i, u in enumerate(meta["utterances"]):
        lp = g["u%d" % i]
        assert lp.shape[0] <= 40 and lp.shape[1] == 45
        (final, status), = nr.nbest(lp[:, None, :], [u["len"]], g[u["lm"]], u["beam"], u["alpha"], meta["blank"], "torch")
        assert status == {None: 0, "IndexError": 1, "ValueError": 2, "KeyError": 3}[u["error"]], i
        assert [ids for ids, _ in final] == u["ids"], i
        if status == 0:
            assert len(final) == u["beam"]
            np.testing.assert_allclose([s for _, s in final], u["scores"], rtol=1e-12, atol=0, err_msg=str(i))
            tied += any(a == b for a, b in zip(u["scores"], u["scores"][1:]))
    assert tied >= 2, "G16 must hold at least two lists with an exact tie"


# ------------------------------------------------------------------------------------------- every decoder case, robustness
def _has_tie(final):
    return any(a[1] == b[1] for a, b in zip(final, final[1:]))


def _check_case(case):
    """Rank 0 / status against oracle.beam, the list length, both exp flavours, the score gaps.  Returns whether a list holds a tie."""
    want, wst, _ = expected(case)
    rows, lists = nr.case_lists(case, "torch")
    _, lists64 = nr.case_lists(case, "f64")
    if case.min_ids:
        assert len(want[0]) > case.min_ids, (case.name, len(want[0]))      # a long-prefix case keeps its long prefixes under a new seed
    tie = False
    for (final, status), (final64, status64), b in zip(lists, lists64, rows):
        assert status == wst[b] == status64, (case.name, b)
        assert [ids for ids, _ in final] == [ids for ids, _ in final64], (case.name, b, "the ranked ids hang on one ulp of exp()")
        if status:
            assert final == []
            continue
        assert len(final) == case.beam and final[0][0] == want[b], (case.name, b)
        for (_, s0), (_, s1) in zip(final, final[1:]):
            assert s0 >= s1
            assert s0 == s1 or (s0 - s1) > 2 * SCORE_RTOL * max(abs(s0), abs(s1)), (case.name, b, s0, s1)
        tie = tie or _has_tie(final)
    return tie


_TIES = {}


@pytest.mark.parametrize("name", [c.name for c in NBEST_CASES])
def test_yardstick_on_every_decoder_case(name):
    _TIES[name] = _check_case(NBEST_BY_NAME[name])


def test_tie_families_show_exact_ties_inside_a_list():
    """Without an exact tie inside a final list the tie rule of the ranking would go untested.  Not every case of these families can hold
    one (beam 1 has a list of one, C 2 a single non-blank class, an LM weight separates group mates, and `mergetie` has its tie at the
    cut of the beam inside the search), so the requirement is on the families: the tied and the uniform family each show lists with
    ties, on both kernels' shapes (fast: beam <= 16 and C <= 64; generic: beyond)."""
    from tests.test_decoders import fast_eligible
    tied = {}
    for case in NBEST_CASES:
        if case.family in TIE_FAMILIES:
            has = _TIES[case.name] if case.name in _TIES else _check_case(case)
            if has:
                tied.setdefault(case.family, set()).add(fast_eligible(case.beam, case.C))
    assert tied.get("tied") == {True, False} and tied.get("uniform") == {True, False}, tied


@pytest.mark.parametrize("beam,Cn", LIMIT_SHAPES)
def test_yardstick_at_the_T_limit(beam, Cn):
    _check_case(LIMIT_CASES[(beam, Cn)])


def test_spread_rows_hit_every_wave_position():
    for case in NBEST_CASES:
        rows = nr.spread_rows(case.B, case.port_rows)
        assert rows[-1] == case.B - 1 and len(set(rows)) == len(rows)
        if case.B > 64:
            assert case.port_rows is not None and len(rows) <= case.port_rows + 1
            for W in (2, 3, 4):
                assert {b % W for b in rows} == set(range(W)), (case.name, W)
            if case.family == "errors":
                assert {b % 12 for b in rows} == set(range(12))
        else:
            assert rows == tuple(range(case.B))


# ---------------------------------------------------------------------------------------------------- host refusals, symbol
def _nbest_args(nbest=None, **over):
    a = list(_beam_args(**over))
    beam = over.get("beam", 10)
    return tuple(a[:9] + [beam if nbest is None else nbest] + a[9:])


_REFUSALS = [p if isinstance(p, dict) else p.values[0] for m in _beam_refusals.pytestmark if m.name == "parametrize" for p in m.args[1]]


def test_the_refusal_list_is_the_beam_entry_s():
    assert len(_REFUSALS) == 17 and dict(beam=65) in _REFUSALS and dict(status=None) in _REFUSALS


@pytest.mark.parametrize("over", _REFUSALS, ids=lambda o: "_".join("%s=%s" % kv for kv in o.items()))
def test_nbest_refuses_what_beam_refuses(over):
    """Refused before any device call (this runs without a GPU), nbest = beam where that is a valid count."""
    L = _L()
    nbest = max(1, min(over.get("beam", 10), 64))
    assert L.mdd_beam_nbest(*_nbest_args(nbest, **over)) == MDD_ERR_ARG
    msg = L.mdd_last_error().decode()
    assert msg.startswith("mdd_beam_nbest"), msg
    if "T" in over and over["T"] > 0 or over.get("C") == 256:
        assert "LDS" in msg and not beam_accepts(over.get("beam", 10), over.get("C", 45), over.get("T", 10)), msg


@pytest.mark.parametrize("nbest,over", [(0, {}), (11, {}), (-1, {}), (2, dict(beam=1)), (65, dict(beam=64)), (5, dict(score=None))],
                         ids=["nbest=0", "nbest=beam+1", "nbest=-1", "beam=1_nbest=2", "beam=64_nbest=65", "score=None"])
def test_nbest_refuses_its_own_bad_arguments(nbest, over):
    L = _L()
    assert L.mdd_beam_nbest(*_nbest_args(nbest, **over)) == MDD_ERR_ARG
    msg = L.mdd_last_error().decode()
    assert msg.startswith("mdd_beam_nbest") and "nbest" in msg, msg


def test_symbol_is_declared_listed_and_exported():
    from ctc_attention_mispronunciation_amd import _lib
    header = open(os.path.join(ROOT, "include", "mdd_hip.h")).read()
    assert re.search(r"\bint mdd_beam_nbest\s*\(", header)
    assert "mdd_beam_nbest" in _lib.EXPORTS and hasattr(_lib.lib(), "mdd_beam_nbest")
    assert _lib.lib().mdd_version() == 100


# ------------------------------------------------------------------------------------------------------- nbest_posteriors
def test_nbest_posteriors():
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import nbest_posteriors
    ll = np.array([-12.5, -13.25, -40.0, -12.5, -800.0])
    e = np.exp(ll - ll.max())
    got = nbest_posteriors(ll)
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, e / e.sum(), rtol=1e-15, atol=0)
    assert abs(got.sum() - 1.0) < 1e-15
    got = nbest_posteriors([-3.0, -np.inf, -4.0])
    assert got[1] == 0.0 and abs(got[0] + got[2] - 1.0) < 1e-15 and got[0] > got[2]
    assert nbest_posteriors([-np.inf, -np.inf]) is None
    assert nbest_posteriors([-np.inf]) is None
    assert nbest_posteriors([-1234.5]).tolist() == [1.0]
    assert nbest_posteriors(np.float32([-2000.0, -2001.0]))[0] == pytest.approx(1.0 / (1.0 + np.exp(-1.0)), rel=1e-15)


# --------------------------------------------------------------------------------------------------------- infer --nbest
def _conf(tmp_path, decode_type, beam_width=10):
    conf = tmp_path / "conf.yaml"
    conf.write_text("exp_name: 'exp'\ncheckpoint_dir: '%s'\nvocab_file: '%s'\nright_ctx: 2\nn_skip_frame: 2\nbatch_size: 4\n"
                    "decode_type: '%s'\nbeam_width: %d\nlm_path: '%s'\nlm_alpha: 0\n"
                    % (tmp_path / "none", tmp_path / "none", decode_type, beam_width, os.path.join(GOLD, "lm_synth45.arpa")))
    return str(conf)


def test_parse_args_takes_nbest():
    from ctc_attention_mispronunciation_amd import infer
    assert infer.parse_args(["--conf", "c", "--wav_transcript_path", "d"]).nbest is None
    assert infer.parse_args(["--conf", "c", "--wav_transcript_path", "d", "--nbest", "3"]).nbest == 3
    with pytest.raises(SystemExit):
        infer.parse_args(["--conf", "c", "--wav_transcript_path", "d", "--nbest", "three"])


@pytest.mark.parametrize("decode_type,n,needle", [("Greedy", 3, "greedy"), ("Beam", 0, "at least 1"), ("Beam", -2, "at least 1"),
                                                  ("Beam", 11, "beam_width = 10")])
def test_main_refuses_nbest(tmp_path, capsys, decode_type, n, needle):
    """Refused through ``refuse`` (status 2, one line on stderr) as soon as the conf is read: before the model, the dictionary and the
    device are touched, and with nothing written into the input folder."""
    from ctc_attention_mispronunciation_amd import infer
    data = tmp_path / "words"
    data.mkdir()
    with pytest.raises(SystemExit) as e:
        infer.main(["--conf", _conf(tmp_path, decode_type), "--wav_transcript_path", str(data), "--nbest", str(n)])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert err.startswith("--nbest") and needle in err and err.count("\n") == 1, err
    assert os.listdir(str(data)) == []
