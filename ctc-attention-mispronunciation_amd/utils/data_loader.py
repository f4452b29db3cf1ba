"""Batch construction at the boundary of the hot path -- mirrors ``utils/data_loader.py`` of the
reference (AA/utils/data_loader.py) for the parts the path needs: ``Vocab`` (units file -> ids,
blank = 0, UNK = 1; :13-52), the context-stack / frame-skip / even-pad of one utterance (:138-142,
done on the GPU by mdd_stack_skip) and the zero-padding collate with its float32 length fractions
(``create_input``, :151-181).  Reading Kaldi ark files is upstream of the path.
``WavBatchLoader`` (inference) and ``TrainWavLoader`` (training, with the reference's augmentation) build the same batches
straight from WAVs on the GPU.
"""
import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .. import _lib


class Vocab(object):
    def __init__(self, vocab_file):
        self.vocab_file = vocab_file
        self.word2index = {"blank": 0, "UNK": 1}
        self.index2word = {0: "blank", 1: "UNK"}
        self.word2count = {}
        self.n_words = 2
        self.read_lang()

    def add_word(self, word):
        if word in self.word2index:
            self.word2count[word] += 1
            return
        self.word2index[word] = self.n_words
        self.index2word[self.n_words] = word
        self.word2count[word] = 1
        self.n_words += 1

    def add_sentence(self, sentence):
        for word in sentence.split(" "):
            self.add_word(word)

    def read_lang(self):
        print("Reading vocabulary from {}".format(self.vocab_file))
        with open(self.vocab_file, "r") as rf:
            for line in rf:
                cols = line.strip().split(" ")
                self.add_sentence(" ".join(cols[1:]) if len(cols) > 1 else cols[0])
        print("Vocabulary size is {}".format(self.n_words))


def stack_features(raw, right_ctx=2, n_skip_frame=2, n_downsample=2, out=None):
    """raw [B, T_raw, D] (or [T_raw, D]) float tensor -> stacked [B, T, (right_ctx+1)*D] on the GPU:
    make_context(feat, 0, right_ctx) + skip_feat(., n_skip_frame) + zero-pad to a multiple of n_downsample."""
    _lib.require_gpu()
    single = raw.dim() == 2
    r = (raw.unsqueeze(0) if single else raw).to("cuda", torch.float32).contiguous()
    B, T_raw, D = r.shape
    T = _lib.lib().mdd_stack_len(T_raw, n_skip_frame, n_downsample)
    if out is None:
        out = torch.empty((B, T, (right_ctx + 1) * D), dtype=torch.float32, device=r.device)
    assert out.is_contiguous() and out.numel() == B * T * (right_ctx + 1) * D
    _lib.check(_lib.lib().mdd_stack_skip(_lib.ptr(r), B, T_raw, D, right_ctx, n_skip_frame, n_downsample, _lib.ptr(out),
                                         _lib.current_stream_ptr()))
    return out.view(T, -1) if single else out.view(B, T, -1)


def frames_from_fraction(input_sizes, t_out):
    """``(input_sizes * probs.size(0)).long()`` of AA/infer.py:296-297 -- float32 multiply, truncation."""
    return (input_sizes.float() * t_out).long()


def create_input(batch):
    """Collate of (feature [T,F], label [n], trans [L], utt) tuples: zero-pad everything to the batch
    maximum; lengths of the features as float32 fractions of the maximum."""
    t_max = max(item[0].size(0) for item in batch)
    n_max = max(item[1].size(0) for item in batch)
    l_max = max(item[2].size(0) for item in batch)
    B, F = len(batch), batch[0][0].size(1)
    data = torch.zeros(B, t_max, F)
    label = torch.zeros(B, n_max)
    trans = torch.zeros(B, l_max)
    in_sizes, lab_sizes, trans_sizes = torch.zeros(B), torch.zeros(B), torch.zeros(B)
    utts = []
    for i, (feat, lab, tr, utt) in enumerate(batch):
        data[i, :feat.size(0)] = feat
        label[i, :lab.size(0)] = lab
        trans[i, :tr.size(0)] = tr
        in_sizes[i] = feat.size(0) / t_max
        lab_sizes[i], trans_sizes[i] = lab.size(0), tr.size(0)
        utts.append(utt)
    return data.float(), in_sizes.float(), label.long(), lab_sizes.long(), trans.long(), trans_sizes.long(), utts


class SpeechDataset(Dataset):
    """Items of one data split: (stacked features [T, (ctx+1)*D], label ids, canonical-transcript ids, utterance id) --
    AA/utils/data_loader.py:54-146 for the fbank feature type.  ``scp_path``: Kaldi scp of ark offsets, ``lab_path`` /
    ``trans_path``: '<utt> <phoneme> <phoneme> ...' lines (annotated and canonical phonemes).  With ``train=True`` every
    item is augmented first (spec_augment on the raw frames, data_enhancement on the canonical ids; :132-137).  The
    stack / skip / even-pad runs on the host here (numpy, as in the reference's loader workers); batches that are already
    on the GPU use ``stack_features`` / ``mdd_forward_raw`` instead."""

    def __init__(self, vocab, scp_path, lab_path, trans_path, opts, train=False):
        self.vocab = vocab
        self.left_ctx, self.right_ctx = opts.left_ctx, opts.right_ctx
        self.n_skip_frame, self.n_downsample = opts.n_skip_frame, opts.n_downsample
        self.train = train
        unk = vocab.word2index["UNK"]

        def ids(path):
            table = {}
            with open(path, "r") as rf:
                for line in rf:
                    if line.strip():
                        utt, text = line.strip().split(" ", 1)
                        table[utt] = [vocab.word2index.get(c, unk) for c in text.split()]
            return table
        paths = []
        with open(scp_path, "r") as rf:
            for line in rf:
                if line.strip():
                    utt, path = line.strip().split(" ")
                    paths.append((utt.split(".")[0], path))
        labels, trans = ids(lab_path), ids(trans_path)
        assert len(paths) == len(labels) == len(trans)
        self.item = [(path, labels[utt], trans[utt], utt) for utt, path in paths]

    def __getitem__(self, idx):
        from .fbank import load_mat
        from .tools import augment_item, make_context, skip_feat
        path, label, trans, utt = self.item[idx]
        feat, trans = augment_item(load_mat(path), trans, train=self.train)
        feat = skip_feat(make_context(feat, self.left_ctx, self.right_ctx), self.n_skip_frame)
        if feat.shape[0] % self.n_downsample:
            feat = np.vstack([feat, np.zeros((self.n_downsample - feat.shape[0] % self.n_downsample, feat.shape[1]))])
        return torch.from_numpy(feat), torch.LongTensor(label), torch.LongTensor(trans), utt

    def __len__(self):
        return len(self.item)


class SpeechDataLoader(DataLoader):
    """DataLoader whose collate is ``create_input`` (AA/utils/data_loader.py:191-194)."""

    def __init__(self, *args, **kwargs):
        super(SpeechDataLoader, self).__init__(*args, **kwargs)
        self.collate_fn = create_input


class WavBatchLoader(object):
    """Batches of WAVs in the shape of ``SpeechDataLoader(SpeechDataset(...), batch_size, shuffle=False)`` as AA/infer.py:278-279
    builds them, straight from samples: ``items`` is a list of (utt, samples [int16 scale], canonical phones as a
    space-separated string[, sample rate, default 16000]), taken in the given order.  Each batch is the reference's 7-tuple
    (inputs, input_sizes, labels, label_sizes, trans, trans_sizes, utt_list): ``inputs`` / ``input_sizes`` come from
    ``fbank.fbank_batch`` (one kernel launch, the features never pass through the host; a batch that holds any rate other than
    16 kHz is first resampled to 16 kHz PCM16 by ``fbank.resample_batch``, AA/infer.py:498-501, and its samples stay on the
    device); trans ids are looked up as SpeechDataset does (unknown -> 'UNK') and padded as create_input pads them; the label pair repeats them (infer.py reads its canonical file as the labels too, :273-276).

    ``pronunciations=True`` (no reference counterpart): an item may carry a fifth entry, the list of all pronunciations of its word (phone
    strings; the first is the item's own), and every batch becomes an 8-tuple whose last entry is ``candidate_sets``' result for it: the
    batch's K = (largest count in the batch) candidate sets for ``CTC_Model.forward_candidates`` and each utterance's count."""

    def __init__(self, items, vocab, batch_size, cmvn=None, right_ctx=2, n_skip_frame=2, n_downsample=2, pronunciations=False):
        self.items = list(items)
        self.vocab = vocab
        self.batch_size = int(batch_size)
        self.cmvn = cmvn
        self.right_ctx, self.n_skip_frame, self.n_downsample = right_ctx, n_skip_frame, n_downsample
        self.pronunciations = bool(pronunciations)

    def __len__(self):
        return (len(self.items) + self.batch_size - 1) // self.batch_size

    def _collate_ids(self, phones):
        """(trans, trans_sizes) of one batch of phone strings, padded to its own longest as create_input pads them."""
        unk = self.vocab.word2index["UNK"]
        ids = [[self.vocab.word2index.get(c, unk) for c in p.split()] for p in phones]
        l_max = max(len(t) for t in ids)
        trans = torch.zeros(len(ids), l_max)
        trans_sizes = torch.zeros(len(ids))
        for i, t in enumerate(ids):
            trans[i, :len(t)] = torch.tensor(t, dtype=torch.float32)
            trans_sizes[i] = len(t)
        return trans.long(), trans_sizes.long()

    def candidate_sets(self, chunk):
        """The candidate sets of one batch of items: ``{"sets": [(trans_k, trans_sizes_k)] * K, "counts": [n_i]}``.  K is the largest number
        of pronunciations an item of the batch carries; set k holds each word's k-th pronunciation, or its first where it has fewer, and is
        padded to its own longest as the reference's collate would pad that batch.  Set 0 is the batch's ordinary ``trans``."""
        prons = [list(it[4]) if len(it) > 4 and it[4] else [it[2]] for it in chunk]
        K = max(len(p) for p in prons)
        return {"sets": [self._collate_ids([p[k] if k < len(p) else p[0] for p in prons]) for k in range(K)], "counts": [len(p) for p in prons]}

    def __iter__(self):
        from .fbank import SAMPLE_RATE, fbank_batch, resample_batch
        for start in range(0, len(self.items), self.batch_size):
            chunk = self.items[start:start + self.batch_size]
            rates = [int(it[3]) if len(it) > 3 else SAMPLE_RATE for it in chunk]
            if all(r == SAMPLE_RATE for r in rates):
                inputs, input_sizes = fbank_batch([it[1] for it in chunk], cmvn=self.cmvn, right_ctx=self.right_ctx,
                                                  n_skip_frame=self.n_skip_frame, n_downsample=self.n_downsample)
            else:
                wav, offsets = resample_batch([it[1] for it in chunk], rates)
                inputs, input_sizes = fbank_batch(wav, cmvn=self.cmvn, right_ctx=self.right_ctx, n_skip_frame=self.n_skip_frame,
                                                  n_downsample=self.n_downsample, offsets=offsets)
            trans, trans_sizes = self._collate_ids([it[2] for it in chunk])
            batch = (inputs, input_sizes, trans.clone(), trans_sizes.clone(), trans, trans_sizes, [it[0] for it in chunk])
            yield batch + (self.candidate_sets(chunk),) if self.pronunciations else batch


def speed_rate(rate, speed):
    """The rate an utterance recorded at ``rate`` Hz is declared to have so that resampling it to 16 kHz plays it ``speed`` times
    as fast (Kaldi-style speed perturbation on the existing resampler): int(round(rate * speed))."""
    return int(round(rate * speed))


class TrainWavLoader(object):
    """Training (and validation) batches straight from WAVs, in the shape and order of ``SpeechDataLoader(SpeechDataset(...,
    train), batch_size, shuffle, num_workers=0)`` as AA/steps/train_ctc.py:131-134 builds them -- the features never exist on
    the host: fbank, CMVN, SpecAugment, context stack, frame skip and padding of a batch are one kernel launch
    (``fbank.fbank_batch``; any rate other than 16 kHz first goes through ``fbank.resample_batch``).

    ``items``: (utt, samples [int16 scale] or the path of a WAV, canonical phones, annotated phones[, sample rate, default 16000]);
    phones are space-separated strings (or lists of names).  A path is read with ``read_wav`` when its batch is formed (its rate
    comes from the file; a 16 kHz file that is not 16-bit PCM is quantised as ``infer.collect`` does).  Each batch is the
    reference's 7-tuple (inputs, input_sizes, labels, label_sizes, trans, trans_sizes, utt_list) with the annotated phones as the
    labels; ids are looked up as SpeechDataset does (unknown -> 'UNK') and padded as create_input pads them.

    Order: torch's own samplers behind a DataLoader over the item indices (RandomSampler or SequentialSampler + BatchSampler, the
    last batch kept), so under one ``torch.manual_seed`` the batches are SpeechDataLoader's.  With ``train=True`` every item gets,
    in batch order, the draws ``tools.augment_item`` makes for it: ``draw_spec_augment(T_raw, 81)`` -- T_raw from the length the
    host already knows -- then ``data_enhancement`` on every canonical id; the spans are applied by the kernel.  ``speeds`` (train
    only), e.g. (0.9, 1.0, 1.1): one factor per item by ``random.choice``, before that item's other draws; an item at rate r and
    speed s is declared to be at ``speed_rate(r, s)`` Hz, so the resampler stretches it, and its T_raw follows ``resample_len``.
    A batch whose declared rates are all 16000 skips the resampler.

    All GPU work goes onto the current stream: no side stream, no thread that launches kernels.  The bf16x3 training step runs
    persistent layer kernels whose workgroups wait on each other; a front-end kernel running beside them could keep one of their
    workgroups off the chip."""

    def __init__(self, items, vocab, batch_size, cmvn=None, right_ctx=2, n_skip_frame=2, n_downsample=2, train=False, shuffle=False,
                 speeds=None):
        self.items = list(items)
        self.vocab = vocab
        self.batch_size = int(batch_size)
        self.cmvn = cmvn
        self.right_ctx, self.n_skip_frame, self.n_downsample = right_ctx, n_skip_frame, n_downsample
        self.train = bool(train)
        self.speeds = list(speeds) if speeds else None
        self._index_batches = DataLoader(range(len(self.items)), batch_size=self.batch_size, shuffle=bool(shuffle), num_workers=0,
                                         collate_fn=list)

    def __len__(self):
        return len(self._index_batches)

    def _ids(self, phones):
        unk = self.vocab.word2index["UNK"]
        return [self.vocab.word2index.get(c, unk) for c in (phones.split() if isinstance(phones, str) else phones)]

    @staticmethod
    def _pad(rows):
        n_max = max(len(r) for r in rows)
        ids, sizes = torch.zeros(len(rows), n_max), torch.zeros(len(rows))
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r, dtype=torch.float32)
            sizes[i] = len(r)
        return ids.long(), sizes.long()

    def __iter__(self):
        import random
        from .fbank import NUM_COLS, SAMPLE_RATE, fbank_batch, quantize_pcm16, read_wav, resample_batch, resample_len
        from .tools import data_enhancement, draw_spec_augment
        L = _lib.lib()
        for index in self._index_batches:
            wavs, rates, labels, trans, utts, fmask, tmask = [], [], [], [], [], [], []
            for k in index:
                it = self.items[int(k)]
                samples, rate = it[1], int(it[4]) if len(it) > 4 else SAMPLE_RATE
                if isinstance(samples, (str, bytes)) or hasattr(samples, "__fspath__"):
                    samples, rate, pcm16 = read_wav(samples, with_format=True)
                    if rate == SAMPLE_RATE and not pcm16:
                        samples = quantize_pcm16(samples)
                n = samples.numel() if torch.is_tensor(samples) else np.asarray(samples).size
                can = self._ids(it[2])
                if self.train:
                    if self.speeds:
                        rate = speed_rate(rate, random.choice(self.speeds))
                    t_raw = L.mdd_fbank_num_frames(resample_len(n, rate))
                    if t_raw == 0:
                        raise ValueError("TrainWavLoader: %s is shorter than one 400-sample window at 16 kHz" % it[0])
                    fs, ts = draw_spec_augment(t_raw, NUM_COLS)
                    fmask.append(fs)
                    tmask.append(ts)
                    can = sum([data_enhancement(t) for t in can], [])
                wavs.append(samples)
                rates.append(rate)
                labels.append(self._ids(it[3]))
                trans.append(can)
                utts.append(it[0])
            kw = dict(cmvn=self.cmvn, right_ctx=self.right_ctx, n_skip_frame=self.n_skip_frame, n_downsample=self.n_downsample)
            if self.train:
                kw.update(fmask=fmask, tmask=tmask)
            if all(r == SAMPLE_RATE for r in rates):
                inputs, input_sizes = fbank_batch(wavs, **kw)
            else:
                wav, offsets = resample_batch(wavs, rates)
                inputs, input_sizes = fbank_batch(wav, offsets=offsets, **kw)
            yield (inputs, input_sizes) + self._pad(labels) + self._pad(trans) + (utts,)
