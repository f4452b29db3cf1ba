"""The float64 references of the best reading of an error network (tests/confnet_best_reference.py) against each other on the CPU, and
the host surface of the feature: the two symbols, the flags of infer and the 'jdiag' / 'jtime' line formatters."""
import os

import numpy as np
import pytest

from tests import confnet_best_reference as best
from tests import confnet_reference as ref
from tests.test_ctc_confnet import tiny_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -np.inf
SYMBOLS = ("mdd_ctc_confnet_best", "mdd_ctc_confnet_best_workspace_bytes")


def close(a, b):
    return abs(a - b) <= 1e-9 * max(1.0, abs(b))


@pytest.mark.parametrize("Cn", (2, 3, 4))
def test_recurrences_against_the_enumeration(Cn):
    feasible = infeasible = 0
    for case in tiny_cases(Cn):
        for b in range(case["lp"].shape[1]):
            lp, w, Tb = case["lp"][:, b, :], case["w"][b, :int(case["nslots"][b])], int(case["lens"][b])
            want, _ = best.brute_best(lp, Tb, w, case["blank"])
            got, reading, seg, path = best.best_f64(lp, Tb, w, case["blank"])
            if np.isneginf(want):
                infeasible += 1
                assert np.isneginf(got) and reading is None, (case["name"], b)
                continue
            feasible += 1
            assert close(got, want), (case["name"], b, got, want)
            # the backtrace is a reading of the network whose best path scores what the sweep found
            again = best.rescore(lp, Tb, w, case["blank"], reading, seg)
            assert again is not None and close(again, got), (case["name"], b, again, got)
            assert list(best.path_of(seg, len(reading), Tb, Tb)) == path, (case["name"], b)
    assert feasible >= 6 and infeasible >= 1


def repeat_network():
    """C = 3, blank 0, two slots offering only label 1 and no skip."""
    w = np.full((2, 3), NEG, np.float32)
    w[:, 1] = 0.0
    return w


def test_repeat_rule():
    lp = ref.posteriors(np.random.default_rng(1), 4, 3)
    lp[1, :] = np.log(np.array([0.01, 0.98, 0.01], np.float32))        # the posteriors favour label 1 in the middle frame
    w = repeat_network()
    assert np.isneginf(best.best_f64(lp, 2, w, 0)[0]) and np.isneginf(best.brute_best(lp, 2, w, 0)[0])
    score, reading, seg, path = best.best_f64(lp, 3, w, 0)
    assert reading == [1, 1] and seg == [[0, 1], [2, 3]] and path == [0, -1, 1]
    assert close(score, float(lp[0, 1]) + float(lp[1, 0]) + float(lp[2, 1]))
    # one slot whose own label is the maximum of the slot in front takes the second maximum: label 2 in front at weight 0 beats label 1
    # there, but slot 1 can only follow it without a blank frame if slot 0 emits something else
    w2 = np.full((2, 3), NEG, np.float32)
    w2[0, 1], w2[0, 2], w2[1, 1] = 0.0, -0.5, 0.0
    lp2 = np.log(np.array([[0.1, 0.8, 0.1], [0.1, 0.8, 0.1]], np.float32))
    score, reading, seg, _ = best.best_f64(lp2, 2, w2, 0)
    want, _ = best.brute_best(lp2, 2, w2, 0)
    assert reading == [2, 1] and seg == [[0, 1], [1, 2]] and close(score, want)
    assert close(score, -0.5 + float(lp2[0, 2]) + float(lp2[1, 1]))


def test_rescore_refuses_what_is_no_reading():
    lp = ref.posteriors(np.random.default_rng(2), 4, 3)
    w = repeat_network()
    assert best.rescore(lp, 3, w, 0, [1, 1], [[0, 1], [2, 3]]) is not None
    assert best.rescore(lp, 3, w, 0, [1, 1], [[0, 1], [1, 2]]) is None          # equal neighbours without a blank frame
    assert best.rescore(lp, 3, w, 0, [1, 2], [[0, 1], [2, 3]]) is None          # no such arc
    assert best.rescore(lp, 3, w, 0, [1, 1], [[0, 2], [1, 3]]) is None          # overlap
    assert best.rescore(lp, 3, w, 0, [1, 1], [[0, 1], [2, 4]]) is None          # past len
    assert best.rescore(lp, 3, w, 0, [1, 0], [[0, 1], [2, 3]]) is None          # no skip arc; and a slot that emits nothing has (-1, -1)
    w[1, 0] = 0.0
    assert best.rescore(lp, 3, w, 0, [1, 0], [[0, 1], [2, 3]]) is None
    assert best.rescore(lp, 3, w, 0, [1, 0], [[0, 1], [-1, -1]]) is not None


def test_symbols_declared_listed_and_exported():
    from ctc_attention_mispronunciation_amd import _lib
    header = open(os.path.join(ROOT, "include", "mdd_hip.h")).read()
    L_ = _lib.lib()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(L_, name), name
    assert L_.mdd_ctc_confnet_best_workspace_bytes(250, 64, 45, 129) > 0
    assert L_.mdd_ctc_confnet_best_workspace_bytes(250, 64, 45, 0) == 0


def test_flag_errors_exit_with_status_2(capsys):
    from ctc_attention_mispronunciation_amd import infer as infer_cli
    from ctc_attention_mispronunciation_amd import infer_core
    base = ["--conf", "no-such-conf.yaml", "--wav_transcript_path", "no-such-folder"]
    for extra in (["--joint_diagnosis"], ["--error_prior", "0.1"], ["--joint_diagnosis", "--error_prior", "0"],
                  ["--joint_diagnosis", "--error_prior", "1"], ["--joint_diagnosis", "--error_prior", "nan"],
                  ["--joint_diagnosis", "--joint_posteriors"]):
        with pytest.raises(SystemExit) as e:
            infer_cli.main(base + extra)
        assert e.value.code == 2, extra
        assert "--error_prior" in capsys.readouterr().err, extra
    args = infer_cli.parse_args(base + ["--joint_diagnosis", "--error_prior", "0.25"])
    assert args.joint_diagnosis and not args.joint_posteriors and args.error_prior == 0.25
    args = infer_cli.parse_args(base + ["--joint_diagnosis", "--joint_posteriors", "--error_prior", "0.25"])
    assert args.joint_diagnosis and args.joint_posteriors and args.error_prior == 0.25
    assert not infer_cli.parse_args(base).joint_diagnosis
    for kw in (dict(error_prior=0.1), dict(joint_diagnosis=True), dict(joint_diagnosis=True, error_prior=1.0)):
        with pytest.raises(ValueError, match="error_prior"):
            infer_core.infer(None, None, [], None, None, None, None, None, False, **kw)


def test_line_formatters():
    from ctc_attention_mispronunciation_amd.infer_core import joint_diagnosis_line, joint_time_line
    names = {0: "<blk>", 1: "k", 2: "ae", 3: "t", 4: "s"}
    ids = [1, 2, 3]
    # k kept, ae substituted by s, t deleted, an s inserted at the end
    diag = ([(1, 0, 2), (4, 3, 5), (0, -1, -1)], [(0, -1, -1), (0, -1, -1), (0, -1, -1), (4, 7, 9)], -12.34567, 0.43219)
    assert joint_diagnosis_line(diag, ids, names) == "jdiag  : k ae>s t>- +s | edits 3 | score -12.3457 | p 0.4322"
    assert joint_time_line(diag, names, 0.04) == "jtime  : k 0.00-0.08 s 0.12-0.20 s 0.28-0.36"
    plain = ([(1, 0, 2), (2, 2, 3), (3, 4, 5)], [(0, -1, -1)] * 4, -1.0, 1.0)
    assert joint_diagnosis_line(plain, ids, names) == "jdiag  : k ae t | edits 0 | score -1.0000 | p 1.0000"
    lead = ([(1, 1, 2)], [(3, 0, 1), (0, -1, -1)], -2.0, 0.5)
    assert joint_diagnosis_line(lead, [1], names, to_display={"K": "K!"}) == "jdiag  : +t K! | edits 1 | score -2.0000 | p 0.5000"
    assert joint_time_line(lead, names, 0.5) == "jtime  : t 0.00-0.50 k 0.50-1.00"
    assert joint_diagnosis_line(None, ids, names) == "jdiag  : -" and joint_time_line(None, names, 0.04) == "jtime  : -"
    with pytest.raises(ValueError):
        joint_diagnosis_line(plain, [1, 2], names)
