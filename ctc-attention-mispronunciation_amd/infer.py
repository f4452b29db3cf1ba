"""Batch inference over a folder of WAVs and word transcripts -- the package's form of the reference's user-facing program
(AA/infer.py:435-598, ``main``), run as

    python -m ctc_attention_mispronunciation_amd.infer --conf CONF --wav_transcript_path DIR [-p cmudict] [-f cmu]
        [--cmvn PATH] [--cmudict PATH] [--precision f32x6|f32|bf16x3] [--decode_seq PATH] [--timestamps] [--posteriors] [--pronunciations] [--nbest N]
        [--mbr N] [--joint_posteriors] [--joint_diagnosis] [--error_prior P]

The conf YAML is read as ``infer_init`` reads it (AA/infer.py:211-261): the checkpoint
``checkpoint_dir/exp_name/ctc_best_model.pkl``, ``vocab_file``, ``decode_type``, ``beam_width``, ``lm_path``, ``lm_alpha``,
``batch_size``, ``right_ctx``, ``n_skip_frame`` (and ``n_downsample``, default 2).  Utterances are the ``N.wav`` files with an
``N.txt`` beside them, in sorted order of ``N`` as a string (the reference takes ``os.listdir`` order; the order changes only
the order of the printed blocks).  The WAVs go to the GPU once and become the padded batches in one kernel launch per batch
(``WavBatchLoader`` / ``fbank_batch``); the loop is ``infer_core.infer``.

WAVs at any rate from 1 to 384 kHz are accepted, in every format ``read_wav`` reads.  As the reference resamples every input
that is not 16 kHz to 16-bit 16 kHz audio (``librosa.resample`` + ``sf.write``, AA/infer.py:498-501), a batch holding such an
input is resampled and quantised to PCM16 on the GPU in one launch (``resample_batch``) and goes on to ``fbank_batch`` without
leaving the device; the reference's rewrite of the input file is not done.  A 16 kHz file that is not 16-bit PCM is
quantised to PCM16 by the same rule on the host (the reference hands it to its denoiser unchanged).  The 3-minute limit, the
400-sample minimum and the total audio time count 16 kHz samples, as the reference counts them after resampling.

What the reference does that needs services absent offline is left out, and says so: no denoiser (``eeo_apm_test``), canonical
phones from the CMU dictionary only (``-p g2p|phonemizer|transcript`` and ``-f ipa`` exit with status 2; a word the dictionary
lacks is skipped with one line), no ECDICT translation (line 4 of each block is empty).  Nothing is written into the input folder.
"""
import argparse
import os
import sys
import time

MAX_SAMPLES = 3 * 60 * 16000          # AA/infer.py:510-512: no more than 3 minutes (the length of its silence.wav)
REFUSED_PHONETIC = {"g2p": "g2p_en", "phonemizer": "phonemizer / espeak", "transcript": "textgrid (TextGrid input)"}


class _Conf(object):
    """steps/train_ctc.py Config: attributes set from the YAML (AA/infer.py:218-220)."""
    batch_size = 4
    dropout = 0.1
    n_downsample = 2


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="infer with only wav and transcript")
    ap.add_argument("--conf", required=True, help="conf file with the checkpoint, vocabulary and decoder settings")
    ap.add_argument("--wav_transcript_path", required=True, help="folder of N.wav / N.txt pairs")
    ap.add_argument("-p", "--phonetic", default="cmudict", help="canonical phone source (only cmudict exists offline)")
    ap.add_argument("-f", "--phonetic_format", default="cmu", help="phone display format (only cmu exists offline)")
    ap.add_argument("--cmvn", default=os.path.join("data", "global_fbank_cmvn.txt"),
                    help="Kaldi global CMVN stats (the reference's data/global_fbank_cmvn.txt)")
    ap.add_argument("--cmudict", default=None, help="CMU pronouncing dictionary (default: dict/cmudict.dict or $MDD_CMUDICT)")
    ap.add_argument("--precision", default=None, choices=("f32x6", "f32", "bf16x3"), help="arithmetic mode of the forward")
    ap.add_argument("--decode_seq", default=None, help="write '<utt> <decoded phones>' lines here")
    ap.add_argument("--timestamps", action="store_true",
                    help="add a 'time   :' line (start-end seconds and confidence per decoded phoneme) and a 'gop    :' line (mean "
                         "log-posterior per canonical phoneme) to each block; times are nominal frame starts")
    ap.add_argument("--posteriors", action="store_true",
                    help="add a 'post   :' line to each block: per canonical phoneme the probability that it was pronounced and the most "
                         "probable alternative (its deletion or a substitute), from the CTC likelihood of every one-edit variant")
    ap.add_argument("--pronunciations", action="store_true",
                    help="score every pronunciation the CMU dictionary lists for the word (word, word(2), ...) on one acoustic pass, report the "
                         "utterance against the one with the highest CTC log-likelihood (not length-normalised; ties go to the earlier entry) "
                         "and add a 'pron   :' line with every pronunciation's log-likelihood")
    ap.add_argument("--nbest", type=int, default=None, metavar="N",
                    help="add N 'nbest  :' lines to each block: the N best final hypotheses of the beam search with their beam score, exact CTC "
                         "log-likelihood, share of probability among the N listed (not an absolute probability) and Comp.; needs "
                         "decode_type Beam and 1 <= N <= beam_width")
    ap.add_argument("--mbr", type=int, default=None, metavar="N",
                    help="add an 'mbr    :' line to each block: the minimum-Bayes-risk hypothesis of the N best final hypotheses of the beam "
                         "search -- the one with the least expected edit distance to the list under the list's own CTC posterior -- with its "
                         "rank, its expected number of phoneme errors (risk), the same for the decoded string (risk1), the list's expected edit "
                         "distance to the canonical phones (exp) and Comp.; the block itself stays the 1-best's.  Needs decode_type Beam and "
                         "2 <= N <= beam_width; independent of --nbest")
    ap.add_argument("--joint_posteriors", action="store_true",
                    help="add a 'jpost  :' line to each block, in the format of 'post   :': the same per-phoneme figures as marginals over the "
                         "error network of the canonical phones -- every phoneme kept, substituted or deleted and every gap empty or filled "
                         "at once -- so two errors in one word no longer count against each other")
    ap.add_argument("--joint_diagnosis", action="store_true",
                    help="add a 'jdiag  :' line to each block: the single most probable combination of kept (ph), substituted (ph>alt), deleted "
                         "(ph>-) and inserted (+ph) phonemes -- decoding constrained to the error network of the canonical phones -- with its "
                         "number of edits, its score and its probability among all readings; with --timestamps a 'jtime  :' line follows with "
                         "the seconds each emitted phoneme occupies.  Needs --error_prior")
    ap.add_argument("--error_prior", type=float, default=None, metavar="P",
                    help="with --joint_posteriors and / or --joint_diagnosis (required by the latter; they share P): prior probability of an "
                         "error per slot, 0 < P < 1 (a position keeps its phoneme with 1 - P and spreads P over the C - 1 other entries; a "
                         "gap stays empty with 1 - P).  Default, --joint_posteriors only: every entry weighs the same")
    return ap.parse_args(argv)


def refuse(msg):
    print(msg, file=sys.stderr)
    sys.exit(2)


def load_model(opts, precision=None):
    """infer_init's checkpoint load (AA/infer.py:227-254) onto the MI355X path.  The class follows the checkpoint: a state_dict without
    ``embeds.weight`` is the CTC-only baseline model (models.cnn_rnn), which recognises without the canonical phones; the rest of the
    program is the same for both, the canonical phones then serving the diagnosis only."""
    import torch
    import torch.nn as nn  # noqa: F401  (a checkpoint pickles nn.LSTM / nn.ReLU by reference)
    if precision is not None:          # read by mdd_create when the model's handle is made
        os.environ["MDD_PRECISION"] = precision
    path = os.path.join(opts.checkpoint_dir, opts.exp_name, "ctc_best_model.pkl")
    package = torch.load(path, map_location="cpu", weights_only=False)
    if "embeds.weight" in package["state_dict"]:
        from .models.model_ctc import CTC_Model
    else:
        from .models.cnn_rnn import CTC_Model
    model = CTC_Model(rnn_param=package["rnn_param"], add_cnn=package["add_cnn"], cnn_param=package["cnn_param"],
                      num_class=package["num_class"], drop_out=package["_drop_out"])
    model.load_state_dict(package["state_dict"])
    model.eval()
    return model


def collect(folder, phonetic, pronunciations=False):
    """(items, word_dict, transcripts, total seconds) over the N.wav / N.txt pairs of `folder`, sorted by N as a string.
    Each item is (utt, samples, phones, sample rate); lengths and seconds are counted at 16 kHz.  ``pronunciations``: the item gets a fifth
    entry, the model phones of every pronunciation ``phonetic.cmu_dict_all`` lists for the word (in dictionary order, the item's own first;
    entries that give the same model phones as an earlier one are dropped), and word_dict[utt]['cmu_all'] their dictionary strings."""
    from .utils.fbank import read_wav, resample_len, quantize_pcm16, SAMPLE_RATE
    items, word_dict, transcripts, total = [], {}, {}, 0.0
    names = sorted(p for p in os.listdir(folder) if os.path.isfile(os.path.join(folder, p)) and p.endswith(".wav"))
    for p in sorted(names, key=lambda q: q[:-4]):
        utt = p[:-4]
        txt = os.path.join(folder, utt + ".txt")
        if not os.path.exists(txt):
            continue
        wav_path = os.path.normpath(os.path.join(folder, p))
        samples, rate, pcm16 = read_wav(wav_path, with_format=True)
        try:
            n16 = resample_len(samples.size, rate)
        except ValueError as e:
            refuse("%s: %s" % (wav_path, e))
        if rate == SAMPLE_RATE and not pcm16:
            samples = quantize_pcm16(samples)
        if n16 > MAX_SAMPLES:
            print("{} skipped, currently wav length should be no more than 3 minutes!".format(wav_path))
            continue
        if n16 < 400:
            print("{} skipped, shorter than one 25 ms window".format(wav_path))
            continue
        with open(txt, "r") as f:
            lines = f.readlines()
        if not lines:
            continue
        utterance = lines[-1].rstrip("\n")
        cmu = phonetic.api_word_phones_cmu(utterance)
        if not cmu:
            print("%s skipped: '%s' is not in the CMU dictionary" % (utt, utterance.strip()))
            continue
        items.append((utt, samples, phonetic.phones_for_model(cmu), rate))
        word_dict[utt] = {"ipa": cmu, "cmu_phns": cmu}
        if pronunciations:
            cmu_all, phones_all = [cmu], [items[-1][2]]
            for alt in phonetic.cmu_dict_all(utterance.strip()):
                if phonetic.phones_for_model(alt) not in phones_all:
                    cmu_all.append(alt)
                    phones_all.append(phonetic.phones_for_model(alt))
            items[-1] += (phones_all,)
            word_dict[utt]["cmu_all"] = cmu_all
        transcripts[utt] = utterance
        total += n16 / float(SAMPLE_RATE)
    return items, word_dict, transcripts, total


def main(argv=None):
    args = parse_args(argv)
    if args.phonetic in REFUSED_PHONETIC:
        refuse("-p %s needs %s, which is not available offline; use -p cmudict" % (args.phonetic, REFUSED_PHONETIC[args.phonetic]))
    if args.phonetic != "cmudict":
        refuse("-p %s: unknown phone source; use -p cmudict" % args.phonetic)
    if args.phonetic_format != "cmu":
        refuse("-f %s needs the IPA tables of phonemizer / espeak, which are not available offline; use -f cmu"
               % args.phonetic_format)
    if args.joint_diagnosis and args.error_prior is None:
        refuse("--joint_diagnosis needs --error_prior P: under the uniform prior a substitution ties with a deletion plus an insertion")
    if args.error_prior is not None:
        if not (args.joint_posteriors or args.joint_diagnosis):
            refuse("--error_prior: only with --joint_posteriors or --joint_diagnosis")
        if not 0.0 < args.error_prior < 1.0:
            refuse("--error_prior %r: P must lie strictly between 0 and 1" % args.error_prior)
    t0 = time.time()
    import yaml
    try:
        conf = yaml.safe_load(open(args.conf, "r"))
    except OSError:
        print("Config file not exist!")
        sys.exit(1)
    opts = _Conf()
    for k, v in conf.items():
        setattr(opts, k, v)
    if args.nbest is not None:
        if opts.decode_type == "Greedy":
            refuse("--nbest: the greedy decoder keeps one hypothesis; set decode_type to Beam")
        if args.nbest < 1:
            refuse("--nbest %d: N must be at least 1" % args.nbest)
        if args.nbest > opts.beam_width:
            refuse("--nbest %d: the search keeps beam_width = %d hypotheses; N cannot exceed it" % (args.nbest, opts.beam_width))
    if args.mbr is not None:
        if opts.decode_type == "Greedy":
            refuse("--mbr: the greedy decoder keeps one hypothesis; set decode_type to Beam")
        if args.mbr < 2:
            refuse("--mbr %d: N must be at least 2 (the risk of a list of one is 0)" % args.mbr)
        if args.mbr > opts.beam_width:
            refuse("--mbr %d: the search keeps beam_width = %d hypotheses; N cannot exceed it" % (args.mbr, opts.beam_width))
    if not os.path.exists(args.cmvn):
        refuse("CMVN stats not found at %s (pass --cmvn)" % args.cmvn)
    print(args.wav_transcript_path, False, args.phonetic)

    from .dict.phonetic_dict import Phonetic
    from .infer_core import infer
    from .utils import fbank
    from .utils.ctcDecoder import GreedyDecoder, BeamDecoder
    from .utils.data_loader import Vocab, WavBatchLoader
    import torch
    phonetic = Phonetic(args.cmudict)
    model = load_model(opts, args.precision)
    vocab = Vocab(opts.vocab_file)
    if opts.decode_type == "Greedy":
        decoder = GreedyDecoder(vocab.index2word, space_idx=-1, blank_index=0)
    else:
        decoder = BeamDecoder(vocab.index2word, beam_width=opts.beam_width, blank_index=0, space_idx=-1, lm_path=opts.lm_path,
                              lm_alpha=opts.lm_alpha)
    t2 = time.time()
    if args.pronunciations and not hasattr(model, "embeds"):
        refuse("--pronunciations: the CTC-only model's posteriors do not depend on the canonical phones; there is nothing to choose between")
    items, word_dict, transcripts, total_wav_time = collect(args.wav_transcript_path, phonetic, args.pronunciations)
    cnt = len(items)
    t3 = time.time()
    cmvn = fbank.cmvn_scale_offset(fbank.read_cmvn_stats(args.cmvn))
    loader = WavBatchLoader(items, vocab, opts.batch_size, cmvn=cmvn, right_ctx=opts.right_ctx, n_skip_frame=opts.n_skip_frame,
                            n_downsample=getattr(opts, "n_downsample", 2), pronunciations=args.pronunciations)
    device = torch.device("cuda", torch.cuda.current_device())
    c1, c2, c3 = infer(phonetic, word_dict, loader, device, model, decoder, vocab, transcripts, False,
                       decode_seq_path=args.decode_seq, timestamps=args.timestamps, posteriors=args.posteriors, pronunciations=args.pronunciations,
                       nbest=args.nbest or 0, joint_posteriors=args.joint_posteriors, error_prior=args.error_prior,
                       joint_diagnosis=args.joint_diagnosis, mbr=args.mbr or 0)
    print(c1, c2, c3)
    end = time.time()
    total = max(total_wav_time, 1e-9)
    rtf = (end - t0) / total
    print("RTF: %.4f, time used for decode %d sentences: %.4f seconds, total wav length: %.4f seconds"
          % (rtf, cnt, end - t0, total_wav_time))
    print("init model time: %.4f, init phone time: %.4f, denoise time: %.4f, mdd infer time: %.4f"
          % ((t2 - t0) / total, (t3 - t2) / total, 0.0, (end - t3) / total))
    print("process time: %.4f" % ((end - t3) / total))
    return 0


if __name__ == "__main__":
    sys.exit(main())
