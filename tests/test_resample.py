"""Any-rate WAV input: the reader (read_wav), the batched GPU resampler to 16 kHz PCM16 (mdd_resample_batch / resample_batch) and the
command-line driver on 44.1 / 48 kHz folders (AA/infer.py:498-501).  ``restate`` below is the float64 numpy restatement of
librosa.resample(kaiser_best) + sf.write's PCM16 quantisation; it runs on the library's own filter table."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import GOLD, ROOT

VOCAB_DIR = os.path.join(GOLD, "vocabulary_single")
RATES = (8000, 11025, 22050, 32000, 44100, 48000, 96000, 12345)


def _fb():
    from ctc_attention_mispronunciation_amd.utils import fbank
    return fbank


def restate(x, fs):
    """Samples on the int16 scale at fs Hz -> the float32 PCM16 values at 16 kHz (the kernel's spec, step by step in float64)."""
    x = np.asarray(x, dtype=np.float32)
    if fs == 16000:
        return x.copy()
    n = x.size
    ratio = 16000.0 / fs
    n_f, n_out = int(n * ratio), int(np.ceil(n * ratio))
    win, delta = _fb().resample_filter(fs)
    scale = min(1.0, ratio)
    step = int(scale * 512)
    xs = x.astype(np.float64) / 32768.0
    t = np.arange(n_f, dtype=np.int64)
    p = t * fs
    n0 = p // 16000
    frac = scale * ((p % 16000) / 16000.0)
    acc = np.zeros(n_f)
    for side in (0, 1):
        if side:
            frac = scale - frac
        idx = frac * 512
        off = idx.astype(np.int64)
        eta = idx - off
        lim = np.minimum(n0 + 1 if side == 0 else n - n0 - 1, (32769 - off) // step)
        for i in range(int(lim.max()) if n_f else 0):
            m = i < lim
            j = np.where(m, off + i * step, 0)
            xi = np.where(m, n0 - i if side == 0 else n0 + 1 + i, 0)
            acc = np.where(m, acc + (win[j] + eta * delta[j]) * xs[xi], acc)
    out = np.zeros(n_out, dtype=np.float32)
    out[:n_f] = np.clip(np.rint(32767.0 * acc), -32768.0, 32767.0)
    return out


def wav_bytes(values, rate, bits=16, tag=1, channels=1, extensible=False):
    """A WAV file as bytes.  ``values``: [frames] or [frames, channels] integers (PCM) or floats (tag 3) as stored."""
    v = np.asarray(values)
    v = v.reshape(v.shape[0], -1) if v.ndim > 1 else np.repeat(v[:, None], channels, axis=1)
    if channels > 1 and v.shape[1] == 1:
        v = np.repeat(v, channels, axis=1)
    w = bits // 8
    if tag == 3:
        body = v.astype("<f4" if bits == 32 else "<f8").tobytes()
    elif bits == 8:
        body = v.astype(np.uint8).tobytes()
    elif bits == 24:
        u = v.astype(np.int64) & 0xFFFFFF
        body = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8).tobytes()
    else:
        body = v.astype("<i2" if bits == 16 else "<i4").tobytes()
    ch = v.shape[1]
    if extensible:
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, ch, rate, rate * ch * w, ch * w, bits, 22, bits, 0)
        fmt += struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
    else:
        fmt = struct.pack("<HHIIHH", tag, ch, rate, rate * ch * w, ch * w, bits)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    chunks += b"LIST" + struct.pack("<I", 5) + b"INFOx\x00"                # an odd-sized chunk the reader must skip (padded)
    chunks += b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)


def _pcm16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_resample_len_matches_librosa_lengths():
    from ctc_attention_mispronunciation_amd import _lib
    L = _lib.lib()
    ns = [0, 1, 2, 3, 5, 63, 64, 100, 177, 399, 400, 441, 4409, 44100, 44101, 160000, 441000, 480000, 2880000]
    ns += [3 * k for k in range(1, 400)] + [3 * k + 1 for k in (7, 1000, 160001)]      # multiples of 3 at 48 kHz
    for rate in RATES + (1000, 16001, 15999, 44056, 383999, 384000):
        for n in ns:
            ratio = 16000.0 / rate
            want = n if rate == 16000 else int(np.ceil(n * ratio))
            assert L.mdd_resample_len(n, rate) == want, (n, rate)
            assert _fb().resample_len(n, rate) == want
        assert L.mdd_resample_len(1, rate) == (1 if rate == 16000 else int(np.ceil(ratio))) >= 1
    assert all(L.mdd_resample_len(n, 16000) == n for n in ns)
    for bad in (0, 999, 384001, -16000, 2 ** 31 - 1):
        assert L.mdd_resample_len(100, bad) == -1
        with pytest.raises(ValueError):
            _fb().resample_len(100, bad)
    assert L.mdd_resample_len(-1, 44100) == -1


@pytest.mark.parametrize("rate", [8000, 16000, 44100, 48000, 12345, 384000])
def test_filter_table_matches_kaiser_best(rate):
    """The library's table against an independent numpy / scipy construction of resampy's kaiser_best (scipy's I0)."""
    from scipy.signal.windows import kaiser
    N, rolloff = 64 * 512, 0.9475937167399596
    ref = kaiser(2 * N + 1, 14.769656459379492)[N:] * (rolloff * np.sinc(rolloff * np.linspace(0, 64, N + 1)))
    ratio = 16000.0 / rate
    if ratio < 1:
        ref = ref * ratio
    win, delta = _fb().resample_filter(rate)
    assert win.shape == delta.shape == (N + 1,)
    assert float(np.abs(win - ref).max()) <= 1e-15
    np.testing.assert_array_equal(delta[:-1], np.diff(win))
    assert delta[-1] == 0.0 and win[0] == pytest.approx(rolloff * min(1.0, ratio), rel=1e-15)


def test_resample_refuses_bad_arguments():
    """Refusals before any device work: a rate out of range, a short table, B <= 0, null offsets."""
    import ctypes as C
    from ctc_attention_mispronunciation_amd import _lib
    L = _lib.lib()
    w = np.zeros(32769)
    p = C.c_void_p(w.ctypes.data)
    assert L.mdd_resample_filter(999, p, p, 32769) == -1
    assert L.mdd_resample_filter(44100, p, p, 32768) == -1
    assert L.mdd_resample_filter(44100, None, p, 32769) == -1
    assert L.mdd_resample_batch(p, p, p, 0, p, p, None) == -1
    assert L.mdd_resample_batch(p, None, p, 2, p, p, None) == -1
    with pytest.raises(ValueError, match="outside"):
        _fb().resample_batch([np.zeros(10, np.float32)], [500])
    with pytest.raises(ValueError):
        _fb().resample_batch([np.zeros(10, np.float32)], [44100, 48000])


def test_read_wav_formats(tmp_path):
    """read_wav on WAVs written byte by byte: 16-bit PCM as before (the integers), every other format as libsndfile's normalised
    value x 32768 of channel 0."""
    fb = _fb()
    rs = np.random.default_rng(3)
    i16 = rs.integers(-32768, 32768, 257).astype(np.int16)
    i16[:2] = (-32768, 32767)
    u8 = rs.integers(0, 256, 257)
    i24 = rs.integers(-2 ** 23, 2 ** 23, 257)
    i24[:2] = (-2 ** 23, 2 ** 23 - 1)
    i32 = rs.integers(-2 ** 31, 2 ** 31, 257)
    f32 = rs.uniform(-1.2, 1.2, 257).astype(np.float32)
    f64 = rs.uniform(-1, 1, 257)
    cases = {  # name: (bytes, expected float32 samples, rate, is 16-bit PCM)
        "pcm16": (wav_bytes(i16, 16000), i16.astype(np.float32), 16000, True),
        "pcm16_ext": (wav_bytes(i16, 44100, extensible=True), i16.astype(np.float32), 44100, True),
        "pcm8": (wav_bytes(u8, 8000, bits=8), ((u8 - 128) / 128.0 * 32768).astype(np.float32), 8000, False),
        "pcm24": (wav_bytes(i24, 48000, bits=24), (i24 / 2.0 ** 23 * 32768).astype(np.float32), 48000, False),
        "pcm24_ext": (wav_bytes(i24, 96000, bits=24, extensible=True), (i24 / 2.0 ** 23 * 32768).astype(np.float32), 96000, False),
        "pcm32": (wav_bytes(i32, 22050, bits=32), (i32 / 2.0 ** 31 * 32768).astype(np.float32), 22050, False),
        "f32": (wav_bytes(f32, 44100, bits=32, tag=3), (f32.astype(np.float64) * 32768).astype(np.float32), 44100, False),
        "f64": (wav_bytes(f64, 32000, bits=64, tag=3), (f64 * 32768).astype(np.float32), 32000, False),
        "f32_ext": (wav_bytes(f32, 11025, bits=32, tag=3, extensible=True), (f32.astype(np.float64) * 32768).astype(np.float32),
                    11025, False),
        "stereo16": (wav_bytes(np.stack([i16, i16[::-1]], 1), 16000), i16.astype(np.float32), 16000, True),
        "stereo24": (wav_bytes(np.stack([i24, -i24 - 1], 1), 44100, bits=24), (i24 / 2.0 ** 23 * 32768).astype(np.float32),
                     44100, False),
    }
    for name, (data, want, rate, pcm16) in cases.items():
        path = str(tmp_path / (name + ".wav"))
        _write(path, data)
        x, r = fb.read_wav(path)
        assert r == rate and x.dtype == np.float32, name
        np.testing.assert_array_equal(x, want, err_msg=name)
        assert fb.read_wav(path, with_format=True)[2] is pcm16, name
    for i in (1, 7, 20):          # the committed 16-bit fixtures: the integers, as the wave-module reader gave them
        import wave
        path = os.path.join(VOCAB_DIR, "%d.wav" % i)
        with wave.open(path, "rb") as w:
            want = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, w.getnchannels())[:, 0].astype(np.float32)
        x, r = fb.read_wav(path)
        assert r == 16000 and np.array_equal(x, want)
    _write(str(tmp_path / "alaw.wav"), wav_bytes(u8, 8000, bits=8, tag=6))
    with pytest.raises(ValueError, match="unsupported"):
        fb.read_wav(str(tmp_path / "alaw.wav"))


def test_quantize_pcm16():
    x = np.array([0.0, 0.5, 1.5, -0.5, 32767.0, 32768.0, -32768.0, 40000.0, -40000.0, 100.25], np.float32)
    want = np.clip(np.rint(x.astype(np.float64) / 32768.0 * 32767.0), -32768, 32767).astype(np.float32)
    np.testing.assert_array_equal(_fb().quantize_pcm16(x), want)
    assert _fb().quantize_pcm16(x)[5] == 32767.0 and _fb().quantize_pcm16(x)[7] == 32767.0


# ------------------------------------------------------------------------------------------------------------------- GPU
def _signals():
    """(samples, rate) rows of one ragged batch: noise, tones and a full-scale square at every rate, lengths from 1 sample to
    10 s, with 16 kHz pass-through rows among them."""
    rs = np.random.default_rng(11)
    rows = []
    for k, fs in enumerate(RATES):
        for n in (1, 2, 3, 40, 177, int(fs * 0.37) + k):
            rows.append(((rs.standard_normal(n) * 6000).astype(np.float32), fs))
        t = np.arange(int(fs * 0.6)) / fs
        rows.append(((9000 * np.sin(2 * np.pi * 440.0 * t) + 4000 * np.sin(2 * np.pi * 0.41 * fs * t)).astype(np.float32), fs))
        sq = np.where(np.sin(2 * np.pi * 700.0 * t[: int(fs * 0.25)]) >= 0, 32767.0, -32768.0).astype(np.float32)
        rows.append((sq, fs))
        rows.append(((rs.standard_normal(123) * 2000).astype(np.float32), 16000))
    rows.append(((rs.standard_normal(441000) * 5000).astype(np.float32), 44100))                     # 10 s
    rows.append(((rs.standard_normal(160000) * 5000 + 0.25).astype(np.float32), 16000))             # 10 s, not integers
    return rows


@pytest.mark.gpu
def test_resample_batch_bit_identical_to_restatement():
    fb = _fb()
    rows = _signals()
    out, off = fb.resample_batch([r[0] for r in rows], [r[1] for r in rows])
    got = out.cpu().numpy()
    assert off.dtype == torch.int64 and off.shape == (len(rows) + 1,) and int(off[-1]) == got.size
    clipped = 0
    for b, (x, fs) in enumerate(rows):
        want = restate(x, fs)
        seg = got[int(off[b]):int(off[b + 1])]
        assert seg.size == fb.resample_len(x.size, fs), (b, fs)
        bad = np.flatnonzero(seg.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (b, fs, x.size, bad[:5], seg[bad[:5]], want[bad[:5]])
        if fs != 16000 and x.size > 1000 and x.max() == 32767.0:
            clipped += int(np.sum(np.abs(want) >= 32767))
    assert clipped > 0     # the full-scale squares ring past full scale and are clipped


def _tone_amplitude(y, f, fs=16000):
    t = np.arange(y.size) / fs
    return 2.0 / y.size * abs(np.sum(y * np.exp(-2j * np.pi * f * t)))


@pytest.mark.gpu
def test_resample_properties():
    """What does not rest on the restatement: a 1 kHz tone keeps its bin and amplitude, a 9 kHz tone at 48 kHz is stopped, and a
    signal band-limited to 6 kHz agrees with scipy.signal.resample_poly.  The bounds are those of resampy's own filter walk:
    its table step int(scale * 512) (185 at 44.1 kHz, 170 at 48 kHz) is below scale * 512, which stretches the filter by up to
    scale * 512 / step - 1 = 0.41 % (gain) and leaves its stopband about 64 dB down at 9 kHz."""
    from scipy.signal import resample_poly
    from tests.helpers import record_margin
    fb = _fb()
    fs = 44100
    t = np.arange(3 * fs) / fs
    tone = (12000 * np.sin(2 * np.pi * 1000.0 * t + 0.3)).astype(np.float32)
    t48 = np.arange(2 * 48000) / 48000
    alias = (29000 * np.sin(2 * np.pi * 9000.0 * t48)).astype(np.float32)
    rs = np.random.default_rng(5)
    band = sum(a * np.sin(2 * np.pi * f * t + ph) for a, f, ph in zip(rs.uniform(500, 2500, 12), rs.uniform(50, 6000, 12),
                                                                     rs.uniform(0, 6.3, 12))).astype(np.float32)
    out, off = fb.resample_batch([tone, alias, band], [fs, 48000, fs])
    y = out.cpu().numpy().astype(np.float64)
    y_tone, y_alias, y_band = (y[int(off[b]):int(off[b + 1])] for b in range(3))
    mid = y_tone[8000:40000]                              # 2 s away from the edges, a whole number of periods
    spec = np.abs(np.fft.rfft(mid))
    assert int(np.argmax(spec)) == 2000                   # 1000 Hz at 0.5 Hz per bin
    amp = _tone_amplitude(mid, 1000.0) / (12000 * 32767 / 32768)
    stretch = (16000.0 / fs) * 512 / int(16000.0 / fs * 512) - 1
    record_margin("resample_tone_1k_amplitude_rel", abs(amp - 1), stretch)
    assert abs(amp - 1) < stretch, amp
    inner = np.abs(y_alias[400:-400]).max()
    record_margin("resample_9k_at_48k_max_abs_lsb", inner, 29.0)
    assert inner <= 29.0, inner                           # at least 60 dB below the 29000 input
    poly = resample_poly(band.astype(np.float64), 160, 441) * (32767 / 32768)
    d = np.abs(y_band[400:-400] - poly[400:y_band.size - 400]).max() / 32768
    record_margin("resample_band6k_vs_resample_poly_fullscale", d, 2e-3)
    assert d < 2e-3, d


@pytest.mark.gpu
def test_resample_then_fbank_batch_equals_host_route():
    """resample_batch -> fbank_batch on the device samples == fbank_batch on the same samples brought to the host."""
    fb = _fb()
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt")))
    rs = np.random.default_rng(2)
    rates = [44100, 16000, 48000, 8000, 12345, 44100]
    wavs = [(rs.standard_normal(int(r * s)) * 3000).astype(np.float32) for r, s in zip(rates, (1.3, 0.9, 2.0, 0.05, 1.1, 10.0))]
    dev, off = fb.resample_batch(wavs, rates)
    x, s = fb.fbank_batch(dev, cmvn=cmvn, offsets=off)
    host = dev.cpu().numpy()
    segs = [host[int(off[b]):int(off[b + 1])] for b in range(len(wavs))]
    want_x, want_s = fb.fbank_batch(segs, cmvn=cmvn)
    assert torch.equal(x.cpu(), want_x.cpu()) and torch.equal(s, want_s)
    assert np.array_equal(segs[1], wavs[1])


def _cli(args, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "ctc_attention_mispronunciation_amd.infer"] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


def _tree(path):
    out = {}
    for name in sorted(os.listdir(path)):
        with open(os.path.join(path, name), "rb") as f:
            out[name] = f.read()
    return out


def _blocks(stdout):
    """The CLI's output without its first line (the folder path) and the timing lines."""
    lines = stdout.splitlines()[1:]
    return [ln for ln in lines if not ln.startswith(("RTF: ", "init model time", "process time"))]


@pytest.mark.gpu
def test_cli_any_rate_folder(tmp_path):
    """The command over the 20 vocabulary_single words at 44.1 kHz plus two at 48 kHz / 24-bit: exit 0, nothing written into the
    folder, and the same output as on a 16 kHz folder holding the restatement's PCM16 output of the same files."""
    import torch.nn as nn
    from scipy.signal import resample_poly
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    fb = _fb()
    src, ref = tmp_path / "any_rate", tmp_path / "at16k"
    os.makedirs(str(src))
    os.makedirs(str(ref))
    for i in range(1, 23):
        w = i if i <= 20 else (3, 8)[i - 21]
        x16, rate = fb.read_wav(os.path.join(VOCAB_DIR, "%d.wav" % w))
        assert rate == 16000
        shutil.copy(os.path.join(VOCAB_DIR, "%d.txt" % w), str(src / ("%d.txt" % i)))
        shutil.copy(os.path.join(VOCAB_DIR, "%d.txt" % w), str(ref / ("%d.txt" % i)))
        if i <= 20:
            _write(str(src / ("%d.wav" % i)), wav_bytes(_pcm16(resample_poly(x16.astype(np.float64), 441, 160)), 44100))
        else:
            y = np.clip(np.rint(resample_poly(x16.astype(np.float64), 3, 1) * 256), -2 ** 23, 2 ** 23 - 1).astype(np.int64)
            _write(str(src / ("%d.wav" % i)), wav_bytes(y, 48000, bits=24))
        x, fs = fb.read_wav(str(src / ("%d.wav" % i)))
        assert fs == (44100 if i <= 20 else 48000)
        _write(str(ref / ("%d.wav" % i)), wav_bytes(restate(x, fs).astype(np.int16), 16000))
    before = _tree(str(src))
    i2c = synth.phone_table_41()
    (tmp_path / "units").write_text("".join(i2c[i] + "\n" for i in range(2, len(i2c))))
    geom = synth.Geometry(**synth.REFERENCE)
    model = CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=0.2)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(geom, seed=11).items()})
    os.makedirs(str(tmp_path / "ckpt" / "exp"))
    torch.save(CTC_Model.save_package(model), str(tmp_path / "ckpt" / "exp" / "ctc_best_model.pkl"))
    conf = tmp_path / "conf.yaml"
    conf.write_text("exp_name: 'exp'\ncheckpoint_dir: '%s'\nvocab_file: '%s'\nleft_ctx: 0\nright_ctx: 2\nn_skip_frame: 2\n"
                    "n_downsample: 2\nbatch_size: 64\ndecode_type: 'Beam'\nbeam_width: 10\nlm_path: '%s'\nlm_alpha: 0\n"
                    % (tmp_path / "ckpt", tmp_path / "units", os.path.join(GOLD, "lm_synth45.arpa")))
    common = ["--conf", str(conf), "--cmvn", os.path.join(GOLD, "global_fbank_cmvn.txt"),
              "--cmudict", os.path.join(GOLD, "cmudict_subset.dict")]
    got = _cli(common + ["--wav_transcript_path", str(src)], timeout=600)
    assert got.returncode == 0, (got.stdout[-2000:], got.stderr[-4000:])
    assert _tree(str(src)) == before
    want = _cli(common + ["--wav_transcript_path", str(ref)], timeout=600)
    assert want.returncode == 0, (want.stdout[-2000:], want.stderr[-4000:])
    assert "id     : 21" in got.stdout and "12 skipped: 'OPPO' is not in the CMU dictionary" in got.stdout
    assert _blocks(got.stdout) == _blocks(want.stdout)
