"""The conditions under which tests/test_fbank.py's bound on the HIP fbank kernels is legitimate, checked without a GPU:
the two restatements of Kaldi's algorithm agree, a plain float32 implementation needs at most 4 units of the model on every
case (so no GPU limit exceeds 16), the floor is exact, and the bound has teeth -- mutations that today's flat 2e-3 lets through
exceed four times the GPU limit of a named case."""
import numpy as np
import pytest

from oracle import oracle
from tests import fbank_reference as R
from tests.helpers import record_margin

YARDSTICK_CAP = 4.0
CASE_NAMES = list(R.CASES)


def test_cases_are_the_float32_samples_the_kernel_receives_and_reach_the_edges():
    assert all(x.dtype == np.float32 and x.ndim == 1 for x in R.CASES.values())
    frames = {name: R.num_frames(x.size) for name, x in R.CASES.items()}
    assert frames["length_399"] == 0 and frames["length_400"] == 1 and frames["length_560"] == 2 and frames["length_1040"] == 5
    assert all(t <= 25 for name, t in frames.items() if not name.startswith("word_"))
    assert max(frames.values()) == frames["word_1"] == 282
    assert np.abs(R.CASES["noise_int16_full_scale"]).max() > 32000 and np.abs(R.CASES["nyquist_32767"]).max() == 32767
    hit = [int(np.any(fr)) for fr in R.frames_of(R.CASES["impulse_slide_321"])]
    assert hit == [1, 1, 1, 0, 0, 0]
    assert [int(np.any(fr)) for fr in R.frames_of(R.CASES["impulse_slide_401"])] == [0, 1, 1, 0, 0, 0]


def test_independent_triangles_equal_the_oracles():
    """First bin and length identical, weights to one float32 ulp: fbank_reference.mel_triangles against oracle.mel_banks."""
    banks = oracle.mel_banks()
    assert len(banks) == R.BINS
    worst = 0.0
    for b, (first, w) in enumerate(banks):
        idx = np.nonzero(R.MEL_INSIDE[b])[0]
        assert idx[0] == first and len(idx) == len(w) and idx[-1] - idx[0] + 1 == len(w), b
        assert w.dtype == np.float32
        ulps = np.abs(R.MEL32[b, idx].astype(np.float64) - w.astype(np.float64)) / np.spacing(np.abs(w)).astype(np.float64)
        worst = max(worst, float(ulps.max()))
        assert not R.MEL32[b, ~R.MEL_INSIDE[b]].any()
    assert worst <= 1.0, worst


def test_window_and_coefficient_are_kaldis_float_values():
    assert np.array_equal(R.WINDOW, R.WINDOW.astype(np.float32).astype(np.float64))
    assert R.WINDOW[0] == R.WINDOW[-1] == np.float32(0.54 - 0.46) and abs(R.WINDOW[199] - 1.0) < 1e-4
    assert R.PREEMPH == float(np.float32(0.97)) != 0.97
    # Parseval holds for S, and the frame mean and energy are what they say they are
    r = R.fbank64(R.CASES["dc_20000_noise_10"])
    assert np.allclose(r.m, 20000.0, atol=5.0) and r.S.shape == r.m.shape == r.e.shape == (11,) and r.E.shape == (11, 80)
    assert r.logs.shape == (11, 81) and np.array_equal(r.logs[:, 0], np.log(r.e))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_fbank_is_within_the_model_of_fbank64(name):
    """oracle.fbank (float32 with a float64 transform) and fbank64 restate the same text on their own: pinned to each other at
    the yardstick's cap."""
    r, lim, _ = R.reference(name)
    got = oracle.fbank(R.CASES[name])
    assert got.shape == r.logs.shape == (R.num_frames(R.CASES[name].size), R.COLS)
    k = R.ratio(got, r, lim)
    print("%s: oracle.fbank at %.3f model units of fbank64" % (name, k))
    assert k <= YARDSTICK_CAP, k


@pytest.mark.parametrize("name", CASE_NAMES)
def test_plain_float32_needs_at_most_four_units(name):
    """The cap that keeps the GPU bound max(1, 4 * k32) from hiding a failure: with it no case's GPU limit exceeds 16 units."""
    r, lim, k32 = R.reference(name)
    got = R.fbank32(R.CASES[name])
    assert got.dtype == np.float32 and got.shape == r.logs.shape
    worst = float(np.abs(got - r.logs).max()) if got.size else 0.0
    print("%s: fbank32 at %.3f model units, largest distance %.2e" % (name, k32, worst))
    record_margin("fbank_k32_%s" % name, k32, YARDSTICK_CAP)
    assert k32 <= YARDSTICK_CAP, k32
    assert 1.0 <= R.gpu_k(name) <= 4.0 * YARDSTICK_CAP


@pytest.mark.parametrize("name", R.FLOOR_CASES)
def test_floor_cases_are_exactly_the_floor(name):
    r, _, _ = R.reference(name)
    ulp = float(np.spacing(np.float32(abs(R.LOG_FLOOR))))
    assert r.logs.shape == (4, R.COLS)
    assert np.abs(r.logs - R.LOG_FLOOR).max() == 0.0
    assert np.abs(R.fbank32(R.CASES[name]).astype(np.float64) - R.LOG_FLOOR).max() <= ulp


def _mutations():
    b = 40
    one_weight = R.MEL64.copy()
    one_weight[b, np.nonzero(R.MEL_INSIDE[b])[0][1]] *= 1.0 + 1e-3
    gain = np.ones(R.HALF)
    gain[37] = 1.0 + 1e-4
    no_last = R.MEL64.copy()
    for b in range(R.BINS):
        no_last[b, np.nonzero(R.MEL_INSIDE[b])[0][-1]] = 0.0
    # (name, keyword arguments of fbank64, the named case, whether today's flat 2e-3 lets it through on that case)
    return [("one_mel_weight_1e-3", dict(weights=one_weight), "noise_3000", True),
            ("one_power_bin_1e-4", dict(power_gain=gain), "word_1", True),
            ("window_period_N", dict(window=R.hamming(R.N)), "impulse_at_0", True),
            ("first_sample_unemphasised", dict(first_sample_rule=False), "impulse_at_0", False),
            ("preemphasis_0.96", dict(preemph=0.96), "tone_93.75Hz", False),
            ("last_triangle_weight_dropped", dict(weights=no_last), "word_1", False)]


@pytest.mark.parametrize("mutation,kwargs,name,passes_today", _mutations(), ids=[m[0] for m in _mutations()])
def test_bound_has_teeth(mutation, kwargs, name, passes_today):
    """A subtly wrong fbank64 exceeds four times the GPU limit of the named case; the first three sit under the flat 2e-3 of
    test_fbank_kernel_against_oracle on that same case (both of its input classes are among them)."""
    r, lim, _ = R.reference(name)
    wrong = R.fbank64(R.CASES[name], **kwargs).logs
    dist = np.abs(wrong - r.logs)
    times = float((dist / (R.gpu_k(name) * lim)).max())
    print("%s on %s: %.1f times the GPU limit (k = %.2f), largest distance %.2e" % (mutation, name, times, R.gpu_k(name), dist.max()))
    record_margin("fbank_teeth_%s_on_%s" % (mutation, name), times)
    assert times >= 4.0, times
    if passes_today:
        assert dist.max() < 2e-3, dist.max()


def test_cmvn_limit_carries_the_log_limit_through_the_scale():
    r, lim, _ = R.reference("noise_3000")
    scale = np.linspace(0.2, 0.5, R.COLS).astype(np.float32)
    offset = np.linspace(-6.0, -2.0, R.COLS).astype(np.float32)
    y, ylim = R.cmvn64(r.logs, scale, offset), R.cmvn_limit(r.logs, lim, scale, offset)
    assert y.dtype == np.float64 and y.shape == ylim.shape == r.logs.shape
    assert np.all(ylim >= scale * lim) and np.all(ylim <= scale * lim + 3 * R.U * (np.abs(r.logs * scale) + np.abs(offset)))
    # a float32 multiply-add of the float32 yardstick stays inside its own k32 units of the carried limit plus one for the two roundings
    got = R.fbank32(R.CASES["noise_3000"]) * scale + offset
    assert got.dtype == np.float32 and float((np.abs(got - y) / ylim).max()) <= max(1.0, R.reference("noise_3000")[2])
