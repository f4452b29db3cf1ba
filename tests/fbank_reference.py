"""float64 yardstick for the fbank kernels (csrc/fbank.hip), with the error model that says how far a correct float32
implementation may sit from it.  numpy / scipy only; vectorised over frames.

``fbank64`` restates Kaldi's published algorithm (feat/feature-window.cc, feat/mel-computations.cc, feat/feature-fbank.cc) for
the option set of conf/fbank.conf -- 16 kHz, 25 ms / 10 ms frames, snip-edges, no dither, remove-dc-offset, raw log energy in
column 0, pre-emphasis 0.97, Hamming window, 512-point transform, power spectrum, 80 mel triangles from 20 Hz to Nyquist,
log -- in float64 throughout, from the float32 samples the kernel receives.  Three things Kaldi holds in ``BaseFloat`` are part
of the specification rather than rounding, and are therefore float32 values here as well: the Hamming window (computed in
double, stored as float), the mel triangles (computed in float), and the pre-emphasis coefficient 0.97f.  (The coefficient
matters: a low-frequency frame leaves pre-emphasis at 3 % of its size, so the 3e-8 between 0.97 and 0.97f is 1e-6 of the result.)
The triangles are built here on their own, not from ``oracle.mel_banks`` or from the kernel's host code; tests/test_fbank_reference.py
pins the two restatements to each other.  The triangles are badly conditioned in the one function Kaldi leaves to the C library:
a weight is a difference of mel values near 2000 over a spacing of 35, so one ulp of ``logf`` is up to 1e-4 of a weight (glibc's
logf and numpy's float32 log differ in 31 of the 256 mel values).  All three restatements therefore use the correctly rounded
logf -- the float64 log of the float32 argument, rounded to float32 -- which any C library's logf matches in all but rare values.

The model.  With u = 2^-23, for frame f and mel column c (output column c + 1):

    limit(f, c) = k * u * ( |ref| + 1 + sqrt((S_f + m_f^2 * D_c) / max(E_fc, u)) )

``ref`` is the float64 log value, ``E_fc`` the float64 mel energy, ``S_f`` the frame's total power spectrum (two-sided sum of
|X_k|^2 over the 512-point transform), ``m_f`` the frame's mean before DC removal and ``D_c`` the mel-weighted power response of
a constant frame of ones put through pre-emphasis and window.  Where the terms come from: a float32 transform leaves every bin
with an error of a few u * sqrt(S_f / 512) * sqrt(log2 512) whatever the bin's own size, so a mel sum E over bins that hold
almost none of the frame's power carries a relative error of u * sqrt(S_f / E): this is the dynamic range of the format, not a
fault.  The float32 mean is off by about u * m_f, which moves every sample of the frame by that constant and so adds
u * m_f times the constant frame's response to the spectrum: relative u * m_f * sqrt(D_c / E) in the mel sum.  |ref| * u is
the rounding of the stored log, and the 1 stands for the O(u) relative errors of window, power and mel sum.  The floor needs no
mask: below it the kernel returns log(u) exactly, and max(E, u) bounds how far a sum on the other side of u can be.
Column 0 (log of the DC-removed raw energy e_f) has ``1 + sqrt(400 * m_f^2 / max(e_f, u))`` as its condition term: subtracting
the mean rounds each of the 400 samples at u * |m_f|.

``limit`` returns model units (k = 1); callers multiply by their k.
"""
import collections
import os
import wave

import numpy as np
import scipy.fft

from tests.helpers import GOLD

U = float(np.finfo(np.float32).eps)          # 2^-23, FLT_EPSILON: the floor under every log and the unit of the model
N, SHIFT, P, BINS, HALF = 400, 160, 512, 80, 256
COLS = BINS + 1
SAMPLE_RATE = 16000.0
PREEMPH = float(np.float32(0.97))            # BaseFloat preemph_coeff
LOG_FLOOR = float(np.log(U))


def num_frames(n):
    """snip-edges: whole windows only."""
    return 0 if n < N else 1 + (n - N) // SHIFT


def hamming(period=N - 1):
    """FeatureWindowFunction: 0.54 - 0.46 cos(2 pi i / (N - 1)) in double, stored as float.  float64 array of float32 values."""
    i = np.arange(N, dtype=np.float64)
    return (0.54 - 0.46 * np.cos(2.0 * np.pi * i / period)).astype(np.float32).astype(np.float64)


def mel_triangles():
    """MelBanks::MelBanks (no VTLN, htk_mode false) in float32, as one dense [80, 256] float32 matrix plus the membership mask.
    Row b is non-zero on the FFT bins whose mel value lies strictly inside (left_b, right_b)."""
    f32 = np.float32

    def mel(freq):                                   # 1127.0f * logf(1.0f + freq / 700.0f) with a correctly rounded logf
        arg = f32(1.0) + np.asarray(freq, dtype=f32) / f32(700.0)
        return f32(1127.0) * np.log(arg.astype(np.float64)).astype(f32)

    lo, hi = mel(20.0), mel(0.5 * SAMPLE_RATE)
    delta = f32((hi - lo) / f32(BINS + 1))
    b = np.arange(BINS, dtype=f32)
    left = (lo + b * delta)[:, None]
    center = (lo + (b + f32(1.0)) * delta)[:, None]
    right = (lo + (b + f32(2.0)) * delta)[:, None]
    m = mel(f32(SAMPLE_RATE / P) * np.arange(HALF, dtype=f32))[None, :]
    inside = (m > left) & (m < right)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(m <= center, (m - left) / (center - left), (right - m) / (right - center))
    w = np.where(inside, w, f32(0.0)).astype(f32)
    assert w.dtype == np.float32 and inside.any(axis=1).all()
    return w, inside


WINDOW = hamming()
MEL32, MEL_INSIDE = mel_triangles()
MEL64 = MEL32.astype(np.float64)


def frames_of(x):
    """[num_frames, 400] float32: the overlapping windows of the samples, as the kernel reads them."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    idx = SHIFT * np.arange(num_frames(x.size))[:, None] + np.arange(N)[None, :]
    return x[idx]


Fbank64 = collections.namedtuple("Fbank64", "logs E S m e")


def fbank64(x, window=None, weights=None, preemph=PREEMPH, first_sample_rule=True, power_gain=None):
    """float32 samples -> Fbank64(logs [T, 81], E [T, 80] mel energies, S [T] total power spectrum, m [T] frame means,
    e [T] DC-removed raw energies), all float64.  The keyword arguments exist for the mutations of the teeth test: another
    window, other mel weights ([80, 256]), another pre-emphasis coefficient, ``pre[0] = fr[0]`` instead of Kaldi's first-sample
    rule, a gain per power bin ([256])."""
    window = WINDOW if window is None else np.asarray(window, dtype=np.float64)
    weights = MEL64 if weights is None else np.asarray(weights, dtype=np.float64)
    fr = frames_of(x).astype(np.float64)
    m = fr.sum(axis=1) / N
    fr = fr - m[:, None]                                             # remove_dc_offset
    e = (fr * fr).sum(axis=1)                                        # raw_energy: before pre-emphasis and window
    pre = np.empty_like(fr)
    pre[:, 1:] = fr[:, 1:] - preemph * fr[:, :-1]
    pre[:, 0] = fr[:, 0] - preemph * fr[:, 0] if first_sample_rule else fr[:, 0]
    pad = np.zeros((fr.shape[0], P))
    pad[:, :N] = pre * window
    spec = np.fft.rfft(pad, axis=1)
    power = (spec.real ** 2 + spec.imag ** 2)[:, :HALF]              # MelBanks reads bins 0..255
    if power_gain is not None:
        power = power * np.asarray(power_gain, dtype=np.float64)
    E = power @ weights.T
    S = P * (pad * pad).sum(axis=1)                                  # Parseval: the two-sided sum of |X_k|^2
    logs = np.log(np.maximum(np.concatenate([e[:, None], E], axis=1), U))
    return Fbank64(logs, E, S, m, e)


def _constant_response():
    """D_c: the mel energies of a frame of ones that skipped DC removal (0.03 times the window, transformed)."""
    pad = np.zeros(P)
    pad[:N] = (1.0 - PREEMPH) * WINDOW
    spec = np.fft.rfft(pad)
    return MEL64 @ (spec.real ** 2 + spec.imag ** 2)[:HALF]


MEL_DC = _constant_response()


def limit(r):
    """The model of the module docstring in units of k, [T, 81] float64, for an ``Fbank64``."""
    cond0 = 1.0 + np.sqrt(N * r.m ** 2 / np.maximum(r.e, U))
    cond = np.sqrt((r.S[:, None] + (r.m ** 2)[:, None] * MEL_DC[None, :]) / np.maximum(r.E, U))
    return U * (np.abs(r.logs) + 1.0 + np.concatenate([cond0[:, None], cond], axis=1))


def fbank32(x):
    """The plain float32 yardstick: the same steps with every value and every sum in float32 and scipy's float32 transform.
    How far this sits from ``fbank64`` is what float32 costs on a case; the GPU bound is a fixed multiple of it."""
    f32 = np.float32
    fr = frames_of(x)
    m = fr.sum(axis=1, dtype=f32) / f32(N)
    fr = fr - m[:, None]
    e = (fr * fr).sum(axis=1, dtype=f32)
    pre = np.empty_like(fr)
    pre[:, 1:] = fr[:, 1:] - f32(PREEMPH) * fr[:, :-1]
    pre[:, 0] = fr[:, 0] - f32(PREEMPH) * fr[:, 0]
    pad = np.zeros((fr.shape[0], P), dtype=f32)
    pad[:, :N] = pre * WINDOW.astype(f32)
    spec = scipy.fft.rfft(pad, axis=1)
    assert spec.dtype == np.complex64, spec.dtype                    # a float64 transform would flatter the yardstick
    power = (spec.real * spec.real + spec.imag * spec.imag)[:, :HALF]
    E = power @ MEL32.T
    out = np.log(np.maximum(np.concatenate([e[:, None], E], axis=1), f32(U)))
    assert fr.dtype == pre.dtype == power.dtype == E.dtype == out.dtype == np.float32
    return out


def ratio(got, r, lim=None):
    """Largest |got - ref| / limit over all elements, in model units (0 for an empty output)."""
    lim = limit(r) if lim is None else lim
    return float((np.abs(np.asarray(got, dtype=np.float64) - r.logs) / lim).max()) if r.logs.size else 0.0


def cmvn64(vals, scale, offset):
    """apply-cmvn with the float32 scale and offset the kernel is given, in float64."""
    return vals * np.asarray(scale, dtype=np.float64) + np.asarray(offset, dtype=np.float64)


def cmvn_limit(vals, lim, scale, offset):
    """Model units for y = val * scale + offset: the log's own limit carried through the scale, plus one rounding each of the
    product and the sum (or of a fused multiply-add)."""
    scale, offset = np.asarray(scale, dtype=np.float64), np.asarray(offset, dtype=np.float64)
    y = vals * scale + offset
    return np.abs(scale) * lim + U * (np.abs(vals * scale) + np.abs(offset) + np.abs(y))


def read_pcm16(path):
    """16-bit mono PCM WAV -> float32 samples on the int16 scale (what Kaldi's WaveData holds)."""
    with wave.open(path, "rb") as w:
        assert w.getsampwidth() == 2 and w.getnchannels() == 1 and w.getframerate() == 16000, path
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float32)


def _cases():
    f32 = np.float32
    c = collections.OrderedDict()

    def rng(seed):
        return np.random.Generator(np.random.PCG64(seed))

    def gauss(seed, n, amp):
        return rng(seed).standard_normal(n) * amp

    def tone(freq, n=2000, amp=10000.0):
        return amp * np.sin(2.0 * np.pi * freq * np.arange(n) / SAMPLE_RATE)

    def impulse(n, at, amp=20000.0):
        x = np.zeros(n)
        x[at] = amp
        return x

    c["noise_3000"] = gauss(101, 4000, 3000.0)
    c["noise_int16_full_scale"] = rng(102).integers(-32768, 32768, size=2000).astype(np.float64)
    c["noise_1e-2"] = gauss(103, 2000, 1e-2)
    c["noise_1lsb"] = rng(104).integers(-1, 2, size=2000).astype(np.float64)
    c["impulse_at_0"] = impulse(400, 0)
    c["impulse_at_1"] = impulse(400, 1)
    c["impulse_at_399"] = impulse(400, 399)
    c["impulse_slide_401"] = impulse(1200, 401)      # inside the frames that start at 160 and 320; the other four are silence
    c["impulse_slide_321"] = impulse(1200, 321)      # inside the frames that start at 0, 160 and 320
    for i, freq in enumerate((93.75, 1000.0, 3999.0, 7900.0)):
        name = "tone_%gHz" % freq
        c[name] = tone(freq)
        c[name + "_noise_3"] = tone(freq) + gauss(110 + i, 2000, 3.0)
    c["nyquist_32767"] = 32767.0 * (1.0 - 2.0 * (np.arange(1200) % 2))
    c["dc_20000_noise_10"] = 20000.0 + gauss(120, 2000, 10.0)
    c["dc_-30000_noise_3"] = -30000.0 + gauss(121, 2000, 3.0)
    c["floor_zeros"] = np.zeros(1000)
    c["floor_constant_1000"] = np.full(1000, 1000.0)
    c["floor_noise_1e-6"] = gauss(130, 1000, 1e-6)
    for n in (399, 400, 560, 1040):                  # no rows; one wave of a four-wave workgroup; two; a partial second workgroup
        c["length_%d" % n] = gauss(140 + n, n, 3000.0)
    c["word_1"] = read_pcm16(os.path.join(GOLD, "vocabulary_single_1.wav"))
    for i in (7, 13):
        c["word_%d" % i] = read_pcm16(os.path.join(GOLD, "vocabulary_single", "%d.wav" % i))
    return collections.OrderedDict((k, np.ascontiguousarray(v, dtype=f32)) for k, v in c.items())


CASES = _cases()
FLOOR_CASES = ("floor_zeros", "floor_constant_1000", "floor_noise_1e-6")

_MEMO = {}


def reference(name):
    """(Fbank64, limit in model units, fbank32's largest ratio k32) of a case, computed once and shared."""
    if name not in _MEMO:
        r = fbank64(CASES[name])
        lim = limit(r)
        for a in r + (lim,):
            a.setflags(write=False)
        _MEMO[name] = (r, lim, ratio(fbank32(CASES[name]), r, lim))
    return _MEMO[name]


def gpu_k(name):
    """The multiple of the model a GPU result of this case is held to: four times what plain float32 needs, at least 1."""
    return max(1.0, 4.0 * reference(name)[2])
