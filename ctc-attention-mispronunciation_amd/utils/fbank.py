"""WAV -> normalised log-mel features on the GPU: the feature step in front of the hot path.

The reference shells out to prebuilt Kaldi binaries for this (``AA/infer.py:567-574``):

    compute-fbank-feats --config=conf/fbank.conf scp:wav.scp ark:- | apply-cmvn --norm-vars=true data/global_fbank_cmvn.txt ark:- ark:- | copy-feats ark:- ark,scp:fbank.ark,fbank.scp

Here: ``compute_fbank_feats`` (HIP kernel behind ``mdd_fbank``), ``read_cmvn_stats`` / ``cmvn_scale_offset`` (Kaldi text
matrix, ``AA/data/global_fbank_cmvn.txt``), and ``write_ark_scp`` / ``read_ark`` for the Kaldi binary float-matrix wire
format the data loader reads (``kaldiio.load_mat``, ``AA/utils/data_loader.py:129``).  Kaldi's dither (random, default
1.0) is not applied.  Parity with Kaldi is unpinned: there is no Kaldi output here to compare with.
"""
import ctypes as C
import struct

import numpy as np
import torch

from .. import _lib

SAMPLE_RATE = 16000
FRAME_SHIFT_SAMPLES = 160        # Kaldi's 10 ms frame shift at 16 kHz (AA/conf/fbank.conf leaves the default)
NUM_COLS = 81


_WAVE_FORMAT_PCM, _WAVE_FORMAT_IEEE_FLOAT, _WAVE_FORMAT_EXTENSIBLE = 1, 3, 0xFFFE


def read_wav(path, with_format=False):
    """WAV -> (float32 samples of channel 0 on the int16 scale, sample rate), as Kaldi's WaveData holds 16-bit PCM.

    Reads what ``sf.read`` reads in a plain WAV (AA/infer.py:497): 8-bit (unsigned), 16-, 24- and 32-bit PCM, IEEE float32 and
    float64, in a plain or a ``WAVE_FORMAT_EXTENSIBLE`` header.  The value is libsndfile's normalised sample (PCM: the integer
    over 2^(bits-1), 8-bit centred on 128; float: as stored) times 32768, so 16-bit PCM comes back as the integers themselves.
    32-bit PCM and float64 keep float32's 24 significant bits.  ``with_format=True`` adds a third value, True when the file is
    16-bit PCM."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("%s: not a RIFF/WAVE file" % path)
    fmt = body = None
    pos = 12
    while pos + 8 <= len(data) and (fmt is None or body is None):
        cid, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        chunk = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = chunk
        elif cid == b"data":
            body = chunk
        pos += 8 + size + (size & 1)
    if fmt is None or body is None or len(fmt) < 16:
        raise ValueError("%s: no fmt or data chunk" % path)
    tag, channels, rate, _, align, bits = struct.unpack_from("<HHIIHH", fmt, 0)
    if tag == _WAVE_FORMAT_EXTENSIBLE:
        if len(fmt) < 26:
            raise ValueError("%s: truncated WAVE_FORMAT_EXTENSIBLE header" % path)
        tag = struct.unpack_from("<H", fmt, 24)[0]          # the first two bytes of the sub-format GUID
    width = bits // 8
    if channels < 1 or bits % 8 or align != channels * width:
        raise ValueError("%s: unsupported layout (%d channels, %d bits, block align %d)" % (path, channels, bits, align))
    frames = len(body) // align
    raw = np.frombuffer(body, dtype=np.uint8, count=frames * align).reshape(frames, align)[:, :width]
    if tag == _WAVE_FORMAT_PCM and bits == 16:
        x = raw.copy().view("<i2")[:, 0].astype(np.float32)
    elif tag == _WAVE_FORMAT_PCM and bits == 8:
        x = ((raw[:, 0].astype(np.float64) - 128.0) * 256.0).astype(np.float32)
    elif tag == _WAVE_FORMAT_PCM and bits == 24:
        v = raw[:, 0].astype(np.int32) | (raw[:, 1].astype(np.int32) << 8) | (raw[:, 2].astype(np.int32) << 16)
        x = ((v - ((v & 0x800000) << 1)).astype(np.float64) / 256.0).astype(np.float32)
    elif tag == _WAVE_FORMAT_PCM and bits == 32:
        x = (raw.copy().view("<i4")[:, 0].astype(np.float64) / 65536.0).astype(np.float32)
    elif tag == _WAVE_FORMAT_IEEE_FLOAT and bits in (32, 64):
        x = (raw.copy().view("<f4" if bits == 32 else "<f8")[:, 0].astype(np.float64) * 32768.0).astype(np.float32)
    else:
        raise ValueError("%s: unsupported WAV sample format (tag %d, %d bits)" % (path, tag, bits))
    pcm16 = tag == _WAVE_FORMAT_PCM and bits == 16
    return (x, rate, pcm16) if with_format else (x, rate)


def quantize_pcm16(samples):
    """Samples on the int16 scale -> the PCM16 values ``sf.write`` stores for them (AA/infer.py:501): clamp(rint(32767 * x),
    -32768, 32767) of x = samples / 32768, in float64, as float32 (the quantisation resample_batch applies to every output)."""
    x = np.asarray(samples, dtype=np.float64) / 32768.0
    return np.clip(np.rint(x * 32767.0), -32768.0, 32767.0).astype(np.float32)


def read_cmvn_stats(path):
    """Kaldi text matrix ``[ sums.. count \\n sumsq.. 0 ]`` -> float64 array [2, D+1]."""
    txt = open(path).read().replace("[", " ").replace("]", " ")
    rows = [r.split() for r in txt.strip().split("\n") if r.split()]
    return np.array([[float(v) for v in r] for r in rows], dtype=np.float64)


def write_cmvn_stats(path, stats):
    """float64 [2, D+1] -> the Kaldi text matrix ``read_cmvn_stats`` reads (`` [`` / two rows / `` ]``), every value with 17
    significant digits, so that reading it back gives the same float64 bits."""
    stats = np.asarray(stats, dtype=np.float64)
    if stats.ndim != 2 or stats.shape[0] != 2:
        raise ValueError("write_cmvn_stats: expected a [2, D+1] matrix, got %s" % (stats.shape,))
    with open(path, "w") as f:
        f.write(" [\n")
        for r, row in enumerate(stats):
            f.write("  " + " ".join("%.17g" % v for v in row) + (" ]\n" if r == 1 else "\n"))


def cmvn_scale_offset(stats, norm_vars=True):
    """(scale, offset) float32 vectors of ``apply-cmvn`` with global stats: out = feat * scale + offset."""
    D = stats.shape[1] - 1
    count = stats[0, D]
    mean = stats[0, :D] / count
    scale = 1.0 / np.sqrt(np.maximum(stats[1, :D] / count - mean * mean, 1e-20)) if norm_vars else np.ones(D)
    return scale.astype(np.float32), (-mean * scale).astype(np.float32)


def compute_fbank_feats(samples, sample_rate=SAMPLE_RATE, cmvn=None, device=None):
    """[num_frames, 81] float32 CUDA tensor (column 0 log energy, 1..80 log mel) for one utterance.

    ``samples``: 1-D array / tensor on the int16 scale; ``cmvn``: None or the (scale, offset) pair of
    ``cmvn_scale_offset`` -- the normalisation is then fused into the kernel's store.
    """
    _lib.require_gpu()
    if sample_rate != SAMPLE_RATE:
        raise ValueError("compute_fbank_feats expects %d Hz audio (resample first, as AA/infer.py:486-516 does)" % SAMPLE_RATE)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    x = torch.as_tensor(np.asarray(samples, dtype=np.float32) if not torch.is_tensor(samples) else samples).to(dev, torch.float32).contiguous()
    n = _lib.lib().mdd_fbank_num_frames(x.numel())
    out = torch.empty((n, NUM_COLS), dtype=torch.float32, device=dev)
    sc = of = None
    if cmvn is not None:
        sc = torch.as_tensor(cmvn[0]).to(dev, torch.float32).contiguous()
        of = torch.as_tensor(cmvn[1]).to(dev, torch.float32).contiguous()
        if sc.numel() != NUM_COLS or of.numel() != NUM_COLS:
            raise ValueError("cmvn vectors must have %d entries" % NUM_COLS)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mdd_fbank(_lib.ptr(x), x.numel(), _lib.ptr(sc), _lib.ptr(of), _lib.ptr(out), _lib.current_stream_ptr()))
    return out


def write_ark_scp(ark_path, scp_path, feats):
    """Kaldi binary archive of float matrices (``<key> \\0B FM \\4 rows \\4 cols data``) plus its scp index.

    ``feats``: dict utt_id -> [T, D] float32 array / tensor (insertion order kept)."""
    with open(ark_path, "wb") as ark, open(scp_path, "w") as scp:
        for key, m in feats.items():
            a = np.ascontiguousarray(m.detach().cpu().numpy() if torch.is_tensor(m) else m, dtype="<f4")
            ark.write(key.encode() + b" ")
            scp.write("%s %s:%d\n" % (key, ark_path, ark.tell()))
            ark.write(b"\0BFM " + b"\x04" + struct.pack("<i", a.shape[0]) + b"\x04" + struct.pack("<i", a.shape[1]))
            ark.write(a.tobytes())


def read_ark(ark_path):
    """dict utt_id -> float32 [T, D] of a binary float-matrix archive written by Kaldi's copy-feats or ``write_ark_scp``."""
    out = {}
    data = open(ark_path, "rb").read()
    pos = 0
    while pos < len(data):
        sp = data.index(b" ", pos)
        key = data[pos:sp].decode()
        pos = sp + 1
        if data[pos:pos + 6] != b"\0BFM \x04"[:6] or data[pos + 5:pos + 6] != b"\x04":
            raise ValueError("%s: entry %r is not an uncompressed binary float matrix" % (ark_path, key))
        rows = struct.unpack_from("<i", data, pos + 6)[0]
        if data[pos + 10:pos + 11] != b"\x04":
            raise ValueError("%s: malformed header at %r" % (ark_path, key))
        cols = struct.unpack_from("<i", data, pos + 11)[0]
        pos += 15
        out[key] = np.frombuffer(data, dtype="<f4", count=rows * cols, offset=pos).reshape(rows, cols).copy()
        pos += 4 * rows * cols
    return out


def load_mat(spec):
    """One matrix by its scp entry ``<ark path>:<byte offset>`` (what ``kaldiio.load_mat`` does for the reference's data
    loader, AA/utils/data_loader.py:130): uncompressed binary float matrices only."""
    path, _, off = spec.rpartition(":")
    if not path:
        raise ValueError("load_mat expects '<ark>:<offset>', got %r" % spec)
    with open(path, "rb") as f:
        f.seek(int(off))
        head = f.read(15)
        if head[:6] != b"\0BFM \x04"[:6] or head[5:6] != b"\x04" or head[10:11] != b"\x04":
            raise ValueError("%s: not an uncompressed binary float matrix" % spec)
        rows, cols = struct.unpack_from("<i", head, 6)[0], struct.unpack_from("<i", head, 11)[0]
        return np.frombuffer(f.read(4 * rows * cols), dtype="<f4").reshape(rows, cols).copy()


MAX_MASKS = 8                    # spans per utterance and kind that mdd_fbank_batch_aug takes
CMVN_STRIP = 64                  # raw frames one workgroup of the statistics kernel walks (csrc/fbank.hip)


def _span_table(spans, B, name):
    """Per-utterance (start, width) lists (or an int array [B, N, 2]) -> int32 [B, N, 2], short lists padded with empty spans."""
    rows = [np.asarray(r, dtype=np.int64).reshape(-1, 2) for r in spans]
    if len(rows) != B:
        raise ValueError("fbank_batch: %s has %d entries for %d utterances" % (name, len(rows), B))
    N = max([r.shape[0] for r in rows] + [0])
    if N > MAX_MASKS:
        raise ValueError("fbank_batch: %s holds %d spans for one utterance, at most %d" % (name, N, MAX_MASKS))
    table = np.zeros((B, N, 2), dtype=np.int64)
    for b, r in enumerate(rows):
        table[b, :r.shape[0]] = r
    return np.clip(table, -2 ** 31, 2 ** 31 - 1).astype(np.int32)      # (the kernel cuts spans to the matrix anyway)


def fbank_batch(wavs, cmvn=None, right_ctx=2, n_skip_frame=2, n_downsample=2, out=None, offsets=None, fmask=None, tmask=None):
    """B utterances -> the padded model input the reference's infer.py batches from them, in one kernel launch (mdd_fbank_batch):
    fbank + CMVN per utterance, make_context(., 0, right_ctx) + skip_feat(., n_skip_frame) + zero rows up to a multiple of
    n_downsample (AA/utils/data_loader.py:138-142), zero-padded to the longest (create_input, :151-181).

    ``wavs``: list of 1-D sample arrays / tensors at 16 kHz on the int16 scale; ``cmvn``: None or the (scale, offset) pair of
    ``cmvn_scale_offset``.  Returns (inputs [B, T_out, (right_ctx+1)*81] float32 CUDA, input_sizes [B] float32 CPU), where
    input_sizes[b] is create_input's float32 ``feature_length / inputs_max_length``.  Each stored frame is bit-identical to
    ``compute_fbank_feats`` of that utterance.  ``out`` (optional) is written whole, padding included.

    With ``offsets`` ([B+1] int64, host), ``wavs`` is instead one 1-D float32 CUDA tensor holding the B utterances back to back,
    utterance b at [offsets[b], offsets[b+1]) -- what ``resample_batch`` returns; the samples stay on the device.

    ``fmask`` / ``tmask`` (train time; both None: the call above, through mdd_fbank_batch): per utterance a list of (start, width)
    spans, as ``tools.draw_spec_augment`` returns them -- columns and raw frames of the utterance's own [T_raw, 81] matrix that are
    zeroed after CMVN and before the stacking, where SpeechDataset applies ``spec_augment`` (mdd_fbank_batch_aug, same launch)."""
    if offsets is not None:
        offsets = np.asarray(offsets.cpu().numpy() if torch.is_tensor(offsets) else offsets, dtype=np.int64).reshape(-1)
        if not (torch.is_tensor(wavs) and wavs.is_cuda and wavs.dtype == torch.float32 and wavs.dim() == 1):
            raise ValueError("fbank_batch: with offsets, wavs must be one 1-D float32 CUDA tensor")
        if offsets.size < 2 or offsets[0] != 0 or np.any(np.diff(offsets) < 0) or offsets[-1] > wavs.numel():
            raise ValueError("fbank_batch: offsets must rise from 0 to at most %d" % wavs.numel())
        n = np.diff(offsets)
    else:
        if len(wavs) == 0:
            raise ValueError("fbank_batch: empty batch")
        host = [np.asarray(w.detach().cpu().numpy() if torch.is_tensor(w) else w, dtype=np.float32).reshape(-1) for w in wavs]
        n = np.array([h.size for h in host], dtype=np.int64)
    B = len(n)
    if fmask is not None or tmask is not None:
        ft = _span_table(fmask if fmask is not None else [[]] * B, B, "fmask")
        tt = _span_table(tmask if tmask is not None else [[]] * B, B, "tmask")
    L = _lib.lib()
    t_out = L.mdd_fbank_batch_len(n.ctypes.data_as(C.POINTER(C.c_int64)), B, n_skip_frame, n_downsample)
    if t_out < 0:
        short = [b for b in range(B) if n[b] < 400]
        raise ValueError("fbank_batch: utterance %s is shorter than one 400-sample window (%s)"
                         % (short[0] if short else "?", L.mdd_last_error().decode()))
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    if offsets is not None:
        wav = wavs.contiguous()
        if wav.device != dev:
            raise ValueError("fbank_batch: the samples are on %s, the current device is %s" % (wav.device, dev))
        off = torch.from_numpy(offsets).to(dev)
    else:
        offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        wav = torch.from_numpy(np.concatenate(host)).to(dev)
        off = torch.from_numpy(offsets).to(dev)
    W = (right_ctx + 1) * NUM_COLS
    if out is None:
        out = torch.empty((B, t_out, W), dtype=torch.float32, device=dev)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, t_out, W)
    sc = of = None
    if cmvn is not None:
        sc = torch.as_tensor(cmvn[0]).to(dev, torch.float32).contiguous()
        of = torch.as_tensor(cmvn[1]).to(dev, torch.float32).contiguous()
        if sc.numel() != NUM_COLS or of.numel() != NUM_COLS:
            raise ValueError("cmvn vectors must have %d entries" % NUM_COLS)
    if fmask is None and tmask is None:
        _lib.check(L.mdd_fbank_batch(_lib.ptr(wav), _lib.ptr(off), B, t_out, _lib.ptr(sc), _lib.ptr(of), right_ctx, n_skip_frame, n_downsample,
                                     _lib.ptr(out), _lib.current_stream_ptr()))
    else:
        spans = torch.from_numpy(np.concatenate([ft.reshape(-1), tt.reshape(-1)])).to(dev)     # one copy for both tables
        fd = spans[:ft.size] if ft.size else None
        td = spans[ft.size:] if tt.size else None
        _lib.check(L.mdd_fbank_batch_aug(_lib.ptr(wav), _lib.ptr(off), B, t_out, _lib.ptr(sc), _lib.ptr(of), right_ctx, n_skip_frame,
                                         n_downsample, _lib.ptr(out), _lib.ptr(fd), ft.shape[1], _lib.ptr(td), tt.shape[1],
                                         _lib.current_stream_ptr()))
    lens = [L.mdd_stack_len(L.mdd_fbank_num_frames(int(k)), n_skip_frame, n_downsample) for k in n]
    sizes = torch.zeros(B)
    for b in range(B):
        sizes[b] = lens[b] / t_out          # a Python true division stored into float32, as create_input does (:177)
    return out, sizes


def cmvn_stats(wavs_or_batches, batch_size=32, stats=None):
    """Global CMVN statistics of a set of utterances on the GPU (mdd_cmvn_accumulate) -- Kaldi's ``compute-cmvn-stats`` over the
    un-normalised fbank rows, which the reference runs once over its training set (AA/steps/make_feat.sh:24-39): float64 [2, 82],
    row 0 the column sums and the frame count, row 1 the sums of squares and 0; ``cmvn_scale_offset`` takes it, ``write_cmvn_stats``
    stores it.

    ``wavs_or_batches``: an iterable (a generator will do) whose entries are 16 kHz utterances (1-D sample arrays / tensors on the
    int16 scale; gathered ``batch_size`` to a launch) and / or whole batches ``(samples, offsets)`` as ``resample_batch`` returns
    them, the samples on the device.  ``stats``: earlier statistics to go on from.  An utterance shorter than one window adds nothing.
    The sums are fp64 in a fixed order: the same utterances in the same order and batches give the same bits."""
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    acc = torch.zeros((2, NUM_COLS + 1), dtype=torch.float64, device=dev)
    if stats is not None:
        acc.copy_(torch.as_tensor(np.asarray(stats, dtype=np.float64).reshape(2, NUM_COLS + 1)))

    def add(wav, offsets):
        n = np.diff(offsets)
        if n.size == 0 or offsets[0] != 0 or np.any(n < 0) or offsets[-1] > wav.numel():
            raise ValueError("cmvn_stats: offsets must rise from 0 to at most %d" % wav.numel())
        off = torch.from_numpy(offsets).to(dev)
        _lib.check(_lib.lib().mdd_cmvn_accumulate(_lib.ptr(wav), _lib.ptr(off), len(n), int(n.max()), _lib.ptr(acc), _lib.current_stream_ptr()))

    def flush(host):
        if host:
            offsets = np.concatenate([[0], np.cumsum([h.size for h in host])]).astype(np.int64)
            add(torch.from_numpy(np.concatenate(host)).to(dev), offsets)

    host = []
    for entry in wavs_or_batches:
        if isinstance(entry, tuple) and len(entry) == 2 and torch.is_tensor(entry[0]) and entry[0].is_cuda:
            flush(host)
            host = []
            wav, offsets = entry
            if wav.dtype != torch.float32 or wav.dim() != 1 or wav.device != dev:
                raise ValueError("cmvn_stats: a batch's samples must be one 1-D float32 tensor on the current device")
            add(wav.contiguous(), np.asarray(offsets.cpu().numpy() if torch.is_tensor(offsets) else offsets, dtype=np.int64).reshape(-1))
        else:
            host.append(np.asarray(entry.detach().cpu().numpy() if torch.is_tensor(entry) else entry, dtype=np.float32).reshape(-1))
            if len(host) == batch_size:
                flush(host)
                host = []
    flush(host)
    return acc.cpu().numpy()


RESAMPLE_MIN_RATE, RESAMPLE_MAX_RATE = 1000, 384000
RESAMPLE_TABLE = 32769        # entries of the kaiser_best half window (64 zero crossings x 512 + 1)


def resample_len(n, rate):
    """Samples ``n`` samples at ``rate`` Hz become at 16 kHz (librosa's int(ceil(n * 16000 / rate)); n itself at 16 kHz)."""
    m = _lib.lib().mdd_resample_len(int(n), int(rate))
    if m < 0:
        raise ValueError("resample: %d Hz is outside [%d, %d] (or n = %d < 0)" % (rate, RESAMPLE_MIN_RATE, RESAMPLE_MAX_RATE, n))
    return int(m)


def resample_filter(rate):
    """The library's kaiser_best table for ``rate`` (mdd_resample_filter): (win, delta), float64 [32769] each."""
    win, delta = np.zeros(RESAMPLE_TABLE), np.zeros(RESAMPLE_TABLE)
    _lib.check(_lib.lib().mdd_resample_filter(int(rate), _lib.ptr(win), _lib.ptr(delta), RESAMPLE_TABLE))
    return win, delta


def resample_batch(wavs, rates):
    """B utterances at their own rates -> 16 kHz PCM16 samples on the device, in one kernel launch (mdd_resample_batch): what
    the reference's ``librosa.resample(data, orig_sr=fs, target_sr=16000)`` + ``sf.write`` give it (AA/infer.py:498-501).

    ``wavs``: list of 1-D sample arrays / tensors on the int16 scale; ``rates``: their sample rates in Hz (1000..384000).
    Returns (samples, offsets): a 1-D float32 CUDA tensor with the utterances back to back, utterance b at
    [offsets[b], offsets[b+1]), and offsets, an int64 CPU tensor [B+1] -- the input ``fbank_batch(samples, offsets=offsets)``
    takes.  Resampled rows hold integers in [-32768, 32767]; 16 kHz rows are the input's float32 values unchanged."""
    if len(wavs) == 0 or len(wavs) != len(rates):
        raise ValueError("resample_batch: %d utterances and %d rates" % (len(wavs), len(rates)))
    host = [np.asarray(w.detach().cpu().numpy() if torch.is_tensor(w) else w, dtype=np.float32).reshape(-1) for w in wavs]
    r = np.array([int(v) for v in rates], dtype=np.int32)
    n_in = np.array([h.size for h in host], dtype=np.int64)
    n_out = np.array([resample_len(k, v) for k, v in zip(n_in, r)], dtype=np.int64)
    in_off = np.concatenate([[0], np.cumsum(n_in)]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(n_out)]).astype(np.int64)
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    wav = torch.from_numpy(np.concatenate(host)).to(dev)
    d_in, d_out, d_rates = (torch.from_numpy(a).to(dev) for a in (in_off, out_off, r))
    out = torch.empty(int(out_off[-1]), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().mdd_resample_batch(_lib.ptr(wav), _lib.ptr(d_in), _lib.ptr(d_rates), len(host), _lib.ptr(d_out), _lib.ptr(out),
                                             _lib.current_stream_ptr()))
    return out, torch.from_numpy(out_off)
