"""The host side of training from WAVs: SpecAugment's draws without the matrix (``draw_spec_augment`` against ``spec_augment``), the CMVN
text file's round trip, the two new symbols and their argument refusals, the speed-perturbation rate mapping, the train program's conf
refusals.  No GPU."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import GOLD, ROOT

SYMBOLS = ("mdd_fbank_batch_aug", "mdd_cmvn_accumulate")


def _state():
    s = np.random.get_state()
    return random.getstate(), (s[0], s[1].tobytes(), s[2], s[3], s[4])


# ------------------------------------------------------------------------------------------------------------- span drawing
@pytest.mark.parametrize("tau,v", [(5, 81), (37, 81), (200, 81)])
@pytest.mark.parametrize("seed", range(5))
def test_drawn_spans_are_spec_augments_masks(seed, tau, v):
    from ctc_attention_mispronunciation_amd.utils.tools import apply_spans, draw_spec_augment, spec_augment
    x = np.random.RandomState(100 + seed).randn(tau, v).astype(np.float32) + 3.0      # no zero of its own
    random.seed(seed)
    np.random.seed(seed)
    want = spec_augment(x)
    after_augment = _state()
    random.seed(seed)
    np.random.seed(seed)
    fspans, tspans = draw_spec_augment(tau, v)
    after_draw = _state()
    assert len(fspans) == len(tspans) == 1
    np.testing.assert_array_equal(apply_spans(x, fspans, tspans), want)
    assert after_draw == after_augment


def test_draw_raises_where_spec_augment_raises():
    """A tau below the drawn time-mask width: ``random.randint`` on an empty range, in both."""
    from ctc_attention_mispronunciation_amd.utils.tools import draw_spec_augment, spec_augment
    hit = 0
    for seed in range(40):
        outcomes = []
        for fn in (lambda: spec_augment(np.ones((1, 81), np.float32)), lambda: draw_spec_augment(1, 81)):
            random.seed(seed)
            np.random.seed(seed)
            try:
                fn()
                outcomes.append((None, _state()))
            except Exception as e:      # noqa: BLE001 -- whatever the one raises, the other must raise
                outcomes.append((type(e), None))
        assert outcomes[0] == outcomes[1], seed
        hit += outcomes[0][0] is not None
    assert hit > 0                      # widths 2..4 are drawn in most seeds: the raising branch is covered


def test_apply_spans_cuts_spans_to_the_matrix():
    from ctc_attention_mispronunciation_amd.utils.tools import apply_spans
    x = np.ones((6, 81), np.float32)
    np.testing.assert_array_equal(apply_spans(x, [(5, 0), (3, -2)], [(2, 0)]), x)
    got = apply_spans(x, [(-3, 5), (79, 2 ** 31 - 1)], [(-2 ** 31, 2 ** 31 - 1), (5, 100)])
    want = x.copy()
    want[:, 0:2] = 0
    want[:, 79:] = 0
    want[5:] = 0                        # the first time span ends at -1: empty
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------- CMVN file
def test_cmvn_stats_round_trip_is_exact(tmp_path):
    from ctc_attention_mispronunciation_amd.utils.fbank import read_cmvn_stats, write_cmvn_stats
    rng = np.random.RandomState(7)
    stats = rng.randn(2, 82) * 10.0 ** rng.randint(-8, 12, size=(2, 82))
    stats[0, 81], stats[1, 81] = 123457.0, 0.0
    p = str(tmp_path / "cmvn.txt")
    write_cmvn_stats(p, stats)
    back = read_cmvn_stats(p)
    assert back.dtype == np.float64 and back.shape == (2, 82)
    assert back.tobytes() == stats.tobytes()
    lines = open(p).read().split("\n")
    assert lines[0] == " [" and lines[2].endswith(" ]") and lines[3] == "" and len(lines) == 4
    golden = read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt"))
    write_cmvn_stats(p, golden)
    assert read_cmvn_stats(p).tobytes() == golden.tobytes()


# ------------------------------------------------------------------------------------------------------------- symbols, refusals
def test_symbols_declared_listed_and_exported():
    from ctc_attention_mispronunciation_amd import _lib
    header = open(os.path.join(ROOT, "include", "mdd_hip.h")).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(L, name), name


def test_fbank_batch_aug_rejects_bad_arguments_before_device_work():
    """Host addresses stand in for device buffers; every call is refused before any pointer is used."""
    from ctc_attention_mispronunciation_amd import _lib
    L = _lib.lib()
    host = np.zeros(81, np.float32)
    buf = C.c_void_p(host.ctypes.data)
    good = dict(B=2, T_out=10, sc=None, of=None, right=2, skip=2, n_down=2, out=buf, fm=buf, NF=1, tm=buf, NT=1)

    def call(**change):
        a = dict(good, **change)
        return L.mdd_fbank_batch_aug(buf, buf, a["B"], a["T_out"], a["sc"], a["of"], a["right"], a["skip"], a["n_down"], a["out"],
                                     a["fm"], a["NF"], a["tm"], a["NT"], None)
    # what mdd_fbank_batch refuses (tests/test_infer_batch.py)
    for change in (dict(B=0), dict(B=-1), dict(sc=buf), dict(of=buf), dict(right=-1), dict(skip=0), dict(n_down=0), dict(T_out=-1),
                   dict(out=None), dict(B=65536), dict(T_out=2 ** 30, skip=2),
                   # the masks' own
                   dict(NF=-1), dict(NF=9), dict(NT=-1), dict(NT=9), dict(fm=None), dict(tm=None), dict(fm=None, tm=None)):
        assert call(**change) == -1, change
        assert L.mdd_last_error().decode().startswith("mdd_fbank_batch_aug: "), change
    assert "fmask_dev" in (call(fm=None), L.mdd_last_error().decode())[1]
    assert "tmask_dev" in (call(tm=None), L.mdd_last_error().decode())[1]
    assert call(T_out=0) == 0                               # an empty output: nothing to do, as mdd_fbank_batch
    assert call(T_out=0, fm=None, NF=0, tm=None, NT=0) == 0
    assert call(T_out=0, NF=9) == -1                        # the counts are checked first
    assert not host.any()


def test_cmvn_accumulate_rejects_bad_arguments_before_device_work():
    from ctc_attention_mispronunciation_amd import _lib
    L = _lib.lib()
    host = np.zeros(2 * 82, np.float64)
    buf = C.c_void_p(host.ctypes.data)
    for wav, off, B, n, stats in ((buf, buf, 0, 1000, buf), (buf, buf, -1, 1000, buf), (buf, buf, 65536, 1000, buf), (buf, buf, 2, -1, buf),
                                  (None, buf, 2, 1000, buf), (buf, None, 2, 1000, buf), (buf, buf, 2, 1000, None),
                                  (buf, buf, 2, 2 ** 40, buf)):
        assert L.mdd_cmvn_accumulate(wav, off, B, n, stats, None) == -1, (B, n)
        assert L.mdd_last_error().decode().startswith("mdd_cmvn_accumulate: ")
    assert L.mdd_cmvn_accumulate(buf, buf, 2, 399, buf, None) == 0          # nothing reaches one window: no device work, nothing added
    assert not host.any()


def test_fbank_batch_refuses_too_many_spans_on_the_host():
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    with pytest.raises(ValueError, match="at most 8"):
        fb.fbank_batch([np.zeros(1000, np.float32)], fmask=[[(0, 1)] * 9], tmask=[[]])
    with pytest.raises(ValueError, match="tmask has 2 entries for 1 utterances"):
        fb.fbank_batch([np.zeros(1000, np.float32)], fmask=[[]], tmask=[[], []])


# ------------------------------------------------------------------------------------------------------------- speed mapping
def test_speed_rates_and_their_lengths():
    """An utterance at rate r and speed s is declared to be at int(round(r * s)) Hz; its 16 kHz length is resample_len's (librosa's
    int(ceil(n * 16000 / rate)), n itself at 16 kHz), so speed 1.1 shortens it and 0.9 lengthens it by that factor."""
    import math
    from ctc_attention_mispronunciation_amd.utils.data_loader import speed_rate
    from ctc_attention_mispronunciation_amd.utils.fbank import resample_len
    assert [speed_rate(16000, s) for s in (0.9, 1.0, 1.1)] == [14400, 16000, 17600]
    assert [speed_rate(8000, s) for s in (0.9, 1.0, 1.1)] == [7200, 8000, 8800]
    assert speed_rate(44100, 0.9) == 39690 and speed_rate(22050, 1.1) == 24255 and speed_rate(11025, 0.95) == int(round(11025 * 0.95))
    for n in (400, 1360, 16000, 31999, 160001):
        for rate in (16000, 8000, 44100):
            for s in (0.9, 1.0, 1.1):
                r = speed_rate(rate, s)
                want = n if r == 16000 else int(math.ceil(n * (16000.0 / r)))
                assert resample_len(n, r) == want, (n, rate, s)
        assert resample_len(n, speed_rate(16000, 1.1)) < n < resample_len(n, speed_rate(16000, 0.9))
        assert resample_len(n, speed_rate(16000, 1.0)) == n


# ------------------------------------------------------------------------------------------------------------- the program's refusals
def _cli(conf_text, tmp_path):
    conf = tmp_path / "conf.yaml"
    conf.write_text(conf_text)
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "ctc_attention_mispronunciation_amd.steps.train_ctc", "--conf", str(conf)], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=120)


def _files(tmp_path, names):
    for n in names:
        (tmp_path / n).write_text("u0 sil\n")
    return {n: str(tmp_path / n) for n in names}


def test_cli_refuses_confs_without_one_data_route(tmp_path, capsys):
    f = _files(tmp_path, ["units", "scp", "wavscp", "lab", "trans"])
    common = ("vocab_file: '%(units)s'\ntrain_lab_path: '%(lab)s'\ntrain_trans_path: '%(trans)s'\nvalid_lab_path: '%(lab)s'\n"
              "valid_trans_path: '%(trans)s'\ncmvn_path: '%(units)s'\n" % f)
    ark = "train_scp_path: '%(scp)s'\nvalid_scp_path: '%(scp)s'\n" % f
    wav = "train_wav_scp: '%(wavscp)s'\nvalid_wav_scp: '%(wavscp)s'\n" % f
    cases = [(common, "no training data"), (common + ark + wav, "both data routes"),
             (common + "train_wav_scp: '%(wavscp)s'\n" % f, "without its partner"),
             (common.replace(f["lab"], f["lab"] + ".missing") + wav, "train_lab_path: no file"),
             (common.replace(f["trans"], f["trans"] + ".missing") + ark, "train_trans_path: no file"),
             (common.replace("cmvn_path", "other_key") + wav, "cmvn_path")]
    from ctc_attention_mispronunciation_amd.steps import train_ctc
    for text, needle in cases:
        (tmp_path / "conf.yaml").write_text(text)
        with pytest.raises(SystemExit) as e:
            train_ctc.cli(["--conf", str(tmp_path / "conf.yaml")])
        out = capsys.readouterr()
        assert e.value.code == 2, needle
        assert needle in out.err and len(out.err.strip().split("\n")) == 1 and out.out == "", (needle, out)
    r = _cli(cases[1][0], tmp_path)                     # once through ``python -m``: the exit status and the streams of the process
    assert r.returncode == 2 and "both data routes" in r.stderr and r.stdout == "", (r.stdout, r.stderr)
    assert sorted(os.listdir(str(tmp_path))) == sorted(["conf.yaml"] + list(f))
