"""Training from WAVs on the GPU: the augmented batched front end (mdd_fbank_batch_aug) against a numpy composition of
``compute_fbank_feats`` rows, bit for bit; the CMVN statistics kernel (mdd_cmvn_accumulate) against float64 sums; ``TrainWavLoader``
against ``SpeechDataLoader(SpeechDataset(train=True))`` over the same utterances' ark features; speed perturbation composed by hand;
the train program end to end on a temp folder, its checkpoint through ``infer.load_model``."""
import functools
import os
import random
import types
import wave

import numpy as np
import pytest
import torch

from tests.helpers import GOLD

pytestmark = pytest.mark.gpu

LENS = (400, 1360, 2000)                  # T_raw 1, 7 and 11
GUARD = 4096                              # floats on either side of an output that must stay as they were
SENTINEL = -12345.5


def _fb():
    from ctc_attention_mispronunciation_amd.utils import fbank
    return fbank


def _signal(n, seed):
    """Seeded noise plus two tones, on the int16 scale."""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    x = 900.0 * rng.randn(n) + 4000.0 * np.sin(2 * np.pi * (300.0 + 70.0 * seed) * t) + 2500.0 * np.sin(2 * np.pi * (2100.0 + 130.0 * seed) * t + 0.3)
    return np.rint(x).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _recorded():
    wav, rate = _fb().read_wav(os.path.join(GOLD, "vocabulary_single_1.wav"))
    assert rate == 16000 and wav.size >= 8000
    return wav


@functools.lru_cache(maxsize=None)
def _wavs():
    return tuple(_signal(n, 3 + i) for i, n in enumerate(LENS))


@functools.lru_cache(maxsize=None)
def _cmvn():
    fb = _fb()
    return fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt")))


@functools.lru_cache(maxsize=None)
def _rows(with_cmvn):
    """compute_fbank_feats of the three utterances, once per CMVN mode; read only."""
    rows = tuple(_fb().compute_fbank_feats(w, cmvn=_cmvn() if with_cmvn else None).cpu().numpy() for w in _wavs())
    assert [r.shape for r in rows] == [(1, 81), (7, 81), (11, 81)]
    for r in rows:
        r.setflags(write=False)
    return rows


def _stacked(rows, fmask, tmask, right, skip, n_down):
    """The numpy oracle: spans on each [T_raw, 81] matrix, then make_context / skip_feat / even pad / batch pad."""
    from ctc_attention_mispronunciation_amd.utils.tools import apply_spans, make_context, skip_feat
    feats = []
    for r, fs, ts in zip(rows, fmask, tmask):
        f = skip_feat(make_context(apply_spans(r, fs, ts), 0, right), skip)
        if f.shape[0] % n_down:
            f = np.vstack([f, np.zeros((n_down - f.shape[0] % n_down, f.shape[1]), np.float32)])
        feats.append(f.astype(np.float32))
    t_out = max(f.shape[0] for f in feats)
    out = np.zeros((len(feats), t_out, (right + 1) * 81), np.float32)
    for b, f in enumerate(feats):
        out[b, :f.shape[0]] = f
    return out


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32).view(np.uint32)


def _guarded(shape):
    big = torch.full((2 * GUARD + int(np.prod(shape)),), SENTINEL, dtype=torch.float32, device="cuda")
    return big, big[GUARD:GUARD + int(np.prod(shape))].view(*shape)


I31 = 2 ** 31 - 1
# per utterance (T_raw 1, 7, 11): (fmask, tmask)
MASK_SETS = {
    # column 0 (lane 0's energy); 63..66 (the mel[0] / mel[1] split); a span ending at column 81; T_raw = 1 fully masked; raw frame 0 and
    # the last raw frame (its edge repeats); an odd raw frame, which only context slots read when skip is 2
    "edges": ([[(0, 1)], [(63, 4)], [(78, 3)]], [[(0, 1)], [(0, 1), (6, 1)], [(1, 1), (10, 1)]]),
    # two overlapping spans, width 0, spans of different counts per utterance (short lists are padded with empty spans)
    "overlap": ([[(10, 5), (12, 6)], [(20, 0)], [(0, 1), (40, 2), (41, 3)]], [[], [(2, 2), (3, 3)], [(4, 0), (5, 1)]]),
    # negative and huge starts and widths: cut to the matrix, sums past 32 bits, nothing outside the output
    "clamped": ([[(-5, 7), (80, I31)], [(I31, I31), (-I31 - 1, I31)], [(5, -3), (-I31 - 1, -I31 - 1), (79, I31)]],
                [[(-3, 5)], [(5, 1000), (I31, I31)], [(-I31 - 1, I31), (10, I31), (3, -1)]]),
    # eight spans of each kind: the most the entry takes
    "eight": ([[(8 * k, 1) for k in range(8)]] * 3, [[(k, 1) for k in range(0, 16, 2)]] * 3),
}


# ------------------------------------------------------------------------------------------------------------- 1. zero masks
@pytest.mark.parametrize("with_cmvn", [False, True])
def test_no_masks_give_fbank_batchs_bits(with_cmvn):
    fb = _fb()
    cmvn = _cmvn() if with_cmvn else None
    want, want_sizes = fb.fbank_batch(list(_wavs()), cmvn=cmvn)
    got, sizes = fb.fbank_batch(list(_wavs()), cmvn=cmvn, fmask=[[]] * 3, tmask=[[]] * 3)          # NF = NT = 0, NULL pointers
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)) and torch.equal(sizes, want_sizes)
    got, _ = fb.fbank_batch(list(_wavs()), cmvn=cmvn, fmask=[[(3, 0)]] * 3, tmask=None)            # empty spans only
    assert np.array_equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------------------- 2. masks
@pytest.mark.parametrize("right,skip,n_down", [(2, 2, 2), (0, 1, 1), (2, 3, 2)])
@pytest.mark.parametrize("with_cmvn", [False, True])
def test_masked_batch_equals_numpy_composition(with_cmvn, right, skip, n_down):
    fb = _fb()
    rows = _rows(with_cmvn)
    for name, (fmask, tmask) in MASK_SETS.items():
        want = _stacked(rows, fmask, tmask, right, skip, n_down)
        big, out = _guarded(want.shape)
        got, _ = fb.fbank_batch(list(_wavs()), cmvn=_cmvn() if with_cmvn else None, right_ctx=right, n_skip_frame=skip, n_downsample=n_down,
                                out=out, fmask=fmask, tmask=tmask)
        assert got.data_ptr() == out.data_ptr()
        diff = np.argwhere(_bits(got) != want.view(np.uint32))
        assert diff.size == 0, (name, len(diff), diff[:5].tolist())
        host = big.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), name
    unmasked = _stacked(rows, [[]] * 3, [[]] * 3, right, skip, n_down)
    edges = _stacked(rows, *MASK_SETS["edges"], right, skip, n_down)
    assert (edges[0] == 0).all() and (unmasked[0] != 0).any()                # T_raw = 1 fully masked: every edge repeat is zero
    assert (edges != unmasked).sum() > 81                                    # the oracle's masks do reach stored values


# ------------------------------------------------------------------------------------------------------------- 3. statistics
def _ref_stats(wavs):
    """float64 numpy sums of compute_fbank_feats rows, and the sum of |x| per column that the bound scales with, in both rows."""
    ref, mag = np.zeros((2, 82)), np.zeros((2, 82))
    for w in wavs:
        x = _fb().compute_fbank_feats(w).cpu().numpy().astype(np.float64)
        ref[0, :81] += x.sum(0)
        ref[1, :81] += (x * x).sum(0)
        ref[0, 81] += x.shape[0]
        mag[0, :81] += np.abs(x).sum(0)
        mag[1, :81] += np.abs(x).sum(0)
    return ref, mag


def _check_stats(got, ref, mag):
    assert got.dtype == np.float64 and got.shape == (2, 82)
    assert got[0, 81] == ref[0, 81] and got[1, 81] == 0.0
    err = np.abs(got - ref)[:, :81]
    worst = float((err / np.maximum(mag[:, :81], 1e-300)).max())
    print("cmvn stats: worst |got - ref| / sum|x| = %.2e (bound 1e-12)" % worst)
    assert (err <= 1e-12 * mag[:, :81]).all(), worst


def test_cmvn_stats_against_float64_sums():
    fb = _fb()
    strip = fb.CMVN_STRIP
    straddle = [_signal(400 + 160 * (k - 1), 20 + k) for k in (strip - 1, strip, strip + 1)]
    wavs = list(_wavs()) + straddle + [_recorded()[:8000]]
    ref, mag = _ref_stats(wavs)
    assert ref[0, 81] == 1 + 7 + 11 + 3 * strip + 48
    got = fb.cmvn_stats(wavs)
    _check_stats(got, ref, mag)
    again = fb.cmvn_stats(wavs)
    assert again.tobytes() == got.tobytes()                                  # the same inputs, the same bits
    # two successive calls accumulate
    first = fb.cmvn_stats(wavs[:4])
    both = fb.cmvn_stats(wavs[4:], stats=first)
    _check_stats(both, ref, mag)
    ref4, mag4 = _ref_stats(wavs[:4])
    _check_stats(first, ref4, mag4)
    # a whole batch on the device, as resample_batch hands it over
    offsets = np.concatenate([[0], np.cumsum([w.size for w in wavs])]).astype(np.int64)
    dev = torch.from_numpy(np.concatenate(wavs)).cuda()
    assert fb.cmvn_stats([(dev, torch.from_numpy(offsets))]).tobytes() == got.tobytes()
    # shorter than one window: nothing
    short = _signal(399, 9)
    assert not fb.cmvn_stats([short]).any()
    assert fb.cmvn_stats([short, wavs[2]]).tobytes() == fb.cmvn_stats([wavs[2]]).tobytes()
    assert fb.cmvn_stats([short], stats=got).tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------------------- 4. loader parity
LOADER_LENS = (1040, 1360, 2000, 2480, 1200, 3120, 1680)       # T_raw >= 5: spec_augment's time mask (width < 5) always fits


@functools.lru_cache(maxsize=None)
def _corpus():
    """(utts, wavs, canonical strings, annotated strings, units) of the loader tests."""
    from ctc_attention_mispronunciation_amd.synth import phone_table_41
    i2c = phone_table_41()
    phones = [i2c[i] for i in range(3, 44)]
    rng = np.random.RandomState(11)
    utts = ["utt%02d" % i for i in range(len(LOADER_LENS))]
    wavs = [_signal(n, 40 + i) for i, n in enumerate(LOADER_LENS)]
    can = [" ".join(rng.choice(phones, size=10 + i % 4)) for i in range(len(utts))]
    lab = [" ".join(rng.choice(phones, size=3 + i % 3)) for i in range(len(utts))]
    return utts, wavs, can, lab, "".join(i2c[i] + "\n" for i in range(2, len(i2c)))


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _same_batch(a, b, where):
    assert len(a) == len(b) == 7, where
    assert a[0].shape == b[0].shape and np.array_equal(_bits(a[0]), _bits(b[0])), where
    for k in range(1, 6):
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k].cpu()), (where, k)
    assert a[6] == b[6], where


@pytest.mark.parametrize("shuffle", [False, True])
def test_loader_equals_speech_dataset_on_ark_features(tmp_path, shuffle):
    from ctc_attention_mispronunciation_amd.utils.data_loader import SpeechDataLoader, SpeechDataset, TrainWavLoader, Vocab
    fb = _fb()
    utts, wavs, can, lab, units = _corpus()
    fb.write_ark_scp(str(tmp_path / "fbank.ark"), str(tmp_path / "fbank.scp"),
                     {u: fb.compute_fbank_feats(w, cmvn=_cmvn()) for u, w in zip(utts, wavs)})
    (tmp_path / "units").write_text(units)
    (tmp_path / "lab").write_text("".join("%s %s\n" % p for p in zip(utts, lab)))
    (tmp_path / "trans").write_text("".join("%s %s\n" % p for p in zip(utts, can)))
    vocab = Vocab(str(tmp_path / "units"))
    opts = types.SimpleNamespace(left_ctx=0, right_ctx=2, n_skip_frame=2, n_downsample=2)
    ds = SpeechDataset(vocab, str(tmp_path / "fbank.scp"), str(tmp_path / "lab"), str(tmp_path / "trans"), opts, train=True)
    ark = SpeechDataLoader(ds, batch_size=3, shuffle=shuffle, num_workers=0)
    wav = TrainWavLoader(list(zip(utts, wavs, can, lab)), vocab, 3, cmvn=_cmvn(), right_ctx=2, n_skip_frame=2, n_downsample=2, train=True,
                         shuffle=shuffle)
    assert len(wav) == len(ark) == 3
    def states():
        return random.getstate(), np.random.get_state()[1].tobytes(), torch.get_rng_state().numpy().tobytes()
    _seed(5)
    want = [list(ark), None]
    after_first = states()
    want[1] = list(ark)                         # the second epoch goes on from the generators' states, in both
    _seed(5)
    got = [list(wav), None]
    assert states() == after_first
    got[1] = list(wav)
    for epoch in range(2):
        assert len(got[epoch]) == len(want[epoch]) == 3
        for k, (a, b) in enumerate(zip(got[epoch], want[epoch])):
            _same_batch(a, b, (epoch, k))
            assert a[0].is_cuda and not torch.equal(a[2], a[4][:, :a[2].shape[1]])          # the labels are the annotated phones
    got = got[0]
    order = [u for b in got for u in b[6]]
    assert sorted(order) == list(utts) and (order != list(utts)) == shuffle
    plain = {u: [vocab.word2index[c] for c in s.split()] for u, s in zip(utts, can)}
    mutated = sum(int(t[:len(plain[u])].tolist() != plain[u]) for b in got for u, t in zip(b[6], b[4]))
    assert mutated > 0                          # the canonical mutation took part (the masks: compared above, and in the tests of the kernel)
    # eval mode: no draws, the unmasked batch, through mdd_fbank_batch
    _seed(6)
    state = random.getstate()
    plain_loader = TrainWavLoader(list(zip(utts, wavs, can, lab)), vocab, 3, cmvn=_cmvn(), train=False, shuffle=False)
    first = next(iter(plain_loader))
    assert random.getstate() == state
    assert np.array_equal(_bits(first[0]), _bits(fb.fbank_batch(wavs[:3], cmvn=_cmvn())[0]))
    assert [t[:len(plain[u])].tolist() for u, t in zip(first[6], first[4])] == [plain[u] for u in utts[:3]]


# ------------------------------------------------------------------------------------------------------------- 5. speeds
def test_speeds_compose_resampler_and_front_end(tmp_path, monkeypatch):
    from ctc_attention_mispronunciation_amd import _lib
    from ctc_attention_mispronunciation_amd.utils.data_loader import TrainWavLoader, Vocab, speed_rate
    from ctc_attention_mispronunciation_amd.utils.tools import data_enhancement, draw_spec_augment
    fb = _fb()
    utts, wavs, can, lab, units = _corpus()
    (tmp_path / "units").write_text(units)
    vocab = Vocab(str(tmp_path / "units"))
    items = list(zip(utts, wavs, can, lab))[:3]
    items[1] = items[1] + (8000,)               # one item at another rate: 8 kHz, perturbed to 7200 or 8800 Hz
    speeds = (0.9, 1.1)
    _seed(8)
    got = next(iter(TrainWavLoader(items, vocab, 3, cmvn=_cmvn(), train=True, speeds=speeds)))
    _seed(8)
    rates, fmask, tmask, trans = [], [], [], []
    for it in items:
        rates.append(speed_rate(it[4] if len(it) > 4 else 16000, random.choice(speeds)))
        t_raw = _lib.lib().mdd_fbank_num_frames(fb.resample_len(it[1].size, rates[-1]))
        fs, ts = draw_spec_augment(t_raw, 81)
        fmask.append(fs)
        tmask.append(ts)
        trans.append(sum([data_enhancement(vocab.word2index[c]) for c in it[2].split()], []))
    assert rates[0] in (14400, 17600) and rates[1] in (7200, 8800)
    samples, offsets = fb.resample_batch([it[1] for it in items], rates)
    want, want_sizes = fb.fbank_batch(samples, cmvn=_cmvn(), offsets=offsets, fmask=fmask, tmask=tmask)
    assert got[0].shape == want.shape and np.array_equal(_bits(got[0]), _bits(want)) and torch.equal(got[1], want_sizes)
    assert [t[:len(w)].tolist() for t, w in zip(got[4], trans)] == trans
    # speed 1.0 at 16 kHz: the resampler is never called

    def never(*a, **k):
        raise AssertionError("resample_batch called for a batch at 16 kHz")
    monkeypatch.setattr(fb, "resample_batch", never)
    _seed(8)
    unit = next(iter(TrainWavLoader(items[:1] + items[2:], vocab, 2, cmvn=_cmvn(), train=True, speeds=(1.0,))))
    assert unit[0].shape[0] == 2 and bool(torch.isfinite(unit[0]).all())


# ------------------------------------------------------------------------------------------------------------- 6. end to end
def _write_wav(path, samples):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.clip(samples, -32768, 32767).astype("<i2").tobytes())


def test_train_program_from_wavs_to_a_checkpoint_infer_loads(tmp_path, capsys):
    from ctc_attention_mispronunciation_amd import infer
    from ctc_attention_mispronunciation_amd.steps import train_ctc
    from ctc_attention_mispronunciation_amd.utils.data_loader import TrainWavLoader, Vocab
    fb = _fb()
    _, _, can, lab, units = _corpus()
    (tmp_path / "units").write_text(units)
    rec = _recorded()
    frames = 0
    for split, count in (("train", 8), ("dev", 4)):
        os.makedirs(str(tmp_path / split))
        scp, labs, trans = [], [], []
        for i in range(count):
            n = 6400 + 160 * i
            x = rec[300 * i:300 * i + n] + 0.3 * _signal(n, 60 + i) if i % 2 == 0 else _signal(n, 60 + i)
            _write_wav(tmp_path / split / ("%s%d.wav" % (split, i)), x)
            scp.append("%s%d %s\n" % (split, i, tmp_path / split / ("%s%d.wav" % (split, i))))
            labs.append("%s%d %s\n" % (split, i, " ".join(lab[i % len(lab)].split()[:3])))
            trans.append("%s%d %s\n" % (split, i, " ".join(can[i % len(can)].split()[:4])))
            frames += (1 + (n - 400) // 160) if split == "train" else 0
        (tmp_path / split / "wav.scp").write_text("".join(scp))
        (tmp_path / split / "phn_text").write_text("".join(labs))
        (tmp_path / split / "transcript_phn_text").write_text("".join(trans))
    conf = dict(exp_name="exp", checkpoint_dir=str(tmp_path / "ckpt"), vocab_file=str(tmp_path / "units"),
                train_wav_scp=str(tmp_path / "train" / "wav.scp"), train_lab_path=str(tmp_path / "train" / "phn_text"),
                train_trans_path=str(tmp_path / "train" / "transcript_phn_text"),
                valid_wav_scp=str(tmp_path / "dev" / "wav.scp"), valid_lab_path=str(tmp_path / "dev" / "phn_text"),
                valid_trans_path=str(tmp_path / "dev" / "transcript_phn_text"), cmvn_path=str(tmp_path / "cmvn" / "global_fbank_cmvn.txt"),
                left_ctx=0, right_ctx=2, n_skip_frame=2, n_downsample=2, num_workers=0, shuffle_train=True, feature_dim=81,
                output_class_dim=41, mel=False, feature_type="fbank", rnn_input_size=243, rnn_hidden_size=20, rnn_layers=1,
                rnn_type="nn.LSTM", bidirectional=True, batch_norm=True, drop_out=0.2, add_cnn=True, layers=2, channel="[(1, 4), (4, 4)]",
                kernel_size="[(3, 3), (3, 3)]", stride="[(1, 2), (2, 2)]", padding="[(1, 1), (1, 1)]", pooling="None",
                activation_function="relu", use_gpu=True, init_lr=0.001, num_epoches=2, end_adjust_acc=2, lr_decay=0.5, batch_size=4,
                weight_decay=0.0005, seed=1234, verbose_step=1, speed_perturb=[0.9, 1.0, 1.1])
    best = train_ctc.main(conf)
    out = capsys.readouterr().out
    # the statistics file: written first, from the training WAVs
    stats = fb.read_cmvn_stats(conf["cmvn_path"])
    assert stats.shape == (2, 82) and stats[0, 81] == frames and stats[1, 81] == 0 and (stats[1, :81] > 0).all()
    # the reference's lines
    for epoch in (1, 2):
        for line in ("Start training epoch: %d, learning_rate: 0.00100" % epoch, "Epoch = %d, step = 2, total_loss = " % epoch,
                     "Epoch %d Train done, total_loss: " % epoch, "Epoch %d Valid done, total_loss: " % epoch,
                     "epoch %d done, cv acc is: " % epoch):
            assert line in out, line
    assert "adjust_rate_count:0 adjust_time:0" in out and "dev loss: " in out and "End training, best dev loss is: " in out
    assert "Epoch 3" not in out and "Number of parameters " in out
    # the checkpoint, through infer's loader, in eval mode
    assert best == os.path.join(conf["checkpoint_dir"], "exp", "ctc_best_model.pkl") and os.path.isfile(best)
    model = infer.load_model(types.SimpleNamespace(checkpoint_dir=conf["checkpoint_dir"], exp_name="exp"))
    assert not model.training and model.rnn_param["rnn_hidden_size"] == 20
    items = train_ctc.wav_items(conf["valid_wav_scp"], conf["valid_lab_path"], conf["valid_trans_path"])
    batch = next(iter(TrainWavLoader(items, Vocab(conf["vocab_file"]), 4, cmvn=fb.cmvn_scale_offset(stats))))
    logp = model(batch[0], batch[4])
    assert logp.shape == (batch[0].shape[1] // 2, 4, 45) and bool(torch.isfinite(logp).all())
    assert float((logp.exp().sum(-1) - 1).abs().max()) < 1e-4
