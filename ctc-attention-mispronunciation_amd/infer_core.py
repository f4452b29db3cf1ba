"""Per-utterance mispronunciation diagnosis -- the host post-processing of AA/infer.py that turns a
decoded phoneme string and the canonical phoneme string into the printed diagnosis and score.

Reference: AA/infer.py:155-209 (print_aligned_string, align_canonical_decoded), :405-433 (stastics),
:304-342 (sil removal, 'err' stripping, score).  Pure Python per utterance (a sentence of 15-20 words is
past 64 phonemes; the forward accepts up to 1596 at H = 384, include/mdd_hip.h); function names are the reference's so callers can switch by changing the import.

``infer`` is the batch loop around them (AA/infer.py:282-372): model, decoder, diagnosis and the printed block per
utterance, over any loader that yields the reference's 7-tuple (``SpeechDataLoader`` or ``WavBatchLoader``).
"""
import math
import sys

import torch

from .utils.data_loader import frames_from_fraction


def print_aligned_string(s1, s2, l):
    pad = lambda p: p + " " if len(p) == 1 else p   # noqa: E731
    return " ".join(pad(p) for p in s1), " ".join(pad(p) for p in s2), " ".join(s + " " for s in l)


def align_canonical_decoded(s1, s2, l):
    """s1 decoded phones, s2 canonical phones, l the op path of Decoder.wer(decoded, canonical).
    Returns the two sequences padded to the length of the path ('D' placeholder in the decoded row where
    a canonical phone was deleted, 'I' placeholder in the canonical row under an inserted phone), then
    (a) all but one of a run of leading insertions dropped, (b) a leading insertion dropped when it
    merely repeats the first aligned decoded phone."""
    hyp, can, ops = [], [], list(l)
    di = ci = 0
    lead = 0
    for pos, op in enumerate(ops):
        if op == "-" or op == "S":
            hyp.append(s1[di]); can.append(s2[ci]); di += 1; ci += 1
        elif op == "D":
            hyp.append("D"); can.append(s2[ci]); ci += 1
        else:
            hyp.append(s1[di]); can.append("I"); di += 1
            if lead == pos:
                lead += 1
    if lead > 0:
        hyp, can, ops = hyp[lead - 1:], can[lead - 1:], ops[lead - 1:]
    if ops[0] == "I" and can[0] == "I" and len(hyp) >= 2 and hyp[0] == hyp[1]:
        hyp, can, ops = hyp[1:], can[1:], ops[1:]
    return hyp, can, ops


def stastics(dc_path, phones_canonicals, phones_decoded):
    """(insertions, substitutions, deletions): the decoded phone under every 'I', the canonical phone over
    every 'S' and every 'D' (all three rows are index-aligned after align_canonical_decoded)."""
    ins = [phones_decoded[i] for i, op in enumerate(dc_path) if op == "I"]
    sub = [phones_canonicals[i] for i, op in enumerate(dc_path) if op == "S"]
    dele = [phones_canonicals[i] for i, op in enumerate(dc_path) if op not in "-SI"]
    return ins, sub, dele


def pronunciation_score(dc_path, n_insertions):
    """infer.py:338-342: ceil((1 - (DS + min(#ins/4, 0.1*(C+DS))) / (DS + C)) * 100)."""
    ds = sum(1 for c in dc_path if c == "D" or c == "S")
    ok = sum(1 for c in dc_path if c == "-")
    penalty = min(n_insertions / 4, 0.1 * (ok + ds))
    return math.ceil((1 - (ds + penalty) / (ds + ok)) * 100), ok, ds


def strip_sil(phones):
    return [p for p in phones if p != "sil"]


def diagnose(decoded, canonical, decoder, to_display=None):
    """One utterance of the loop at infer.py:304-342.  decoded / canonical: space-separated phoneme strings
    (as the decoders return them).  Returns a dict with the aligned rows, fault lists and score."""
    hyp = " ".join(strip_sil(decoded.split(" ")))
    ref = " ".join(strip_sil(canonical.split(" ")))
    hyp = hyp.replace("err", "").replace("  ", " ")
    _, path = decoder.wer(hyp, ref)
    ph_dec = [c for c in hyp.split(" ") if c]
    ph_can = [c for c in ref.split(" ") if c]
    if to_display is not None:
        ph_dec = [to_display.get(c.upper(), c) for c in ph_dec]
        ph_can = [to_display.get(c.upper(), c) for c in ph_can]
    ph_dec, ph_can, path = align_canonical_decoded(ph_dec, ph_can, path)
    ins, sub, dele = stastics(path, ph_can, ph_dec)
    score, ok, ds = pronunciation_score(path, len(ins))
    return dict(decoded=ph_dec, canonical=ph_can, path=path, insertions=ins, substitutions=sub, deletions=dele,
                correct=ok, del_sub=ds, score=score, printed=print_aligned_string(ph_dec, ph_can, path))


def _tokens(phones):
    return phones.split() if isinstance(phones, str) else [p for p in phones if p]


def diagnose_indexed(decoded_phones, canonical_phones, decoder, to_display=None):
    """``diagnose`` plus, for every row of its ``path``, which token of the inputs the row shows: returns ``(d, rows)`` with rows[r] =
    ``(decoded_index | None, canonical_index | None)`` into the token lists as given (None on the side a 'D' / 'I' row leaves empty).
    The indices follow their tokens through the 'sil' strip, the 'err' removal and the leading-insertion drops of ``diagnose`` /
    ``align_canonical_decoded``, so per-token data of any kind (spans, posteriors) can ride along; a path that does not fit the token
    counts raises ValueError rather than mis-assigning an entry."""
    dec, can = _tokens(decoded_phones), _tokens(canonical_phones)
    d = diagnose(" ".join(dec), " ".join(can), decoder, to_display)
    # the same strip as diagnose, with each token's index carried along ('err' is removed as a substring, as diagnose removes it)
    dec_kept = [i for i, p in enumerate(dec) if p != "sil" and p.replace("err", "")]
    can_kept = [i for i, p in enumerate(can) if p != "sil"]
    hyp = " ".join(dec[i].replace("err", "") for i in dec_kept)
    _, full = decoder.wer(hyp, " ".join(can[i] for i in can_kept))
    dropped = len(full) - len(d["path"])
    if dropped < 0 or list(full[dropped:]) != list(d["path"]) or any(op != "I" for op in full[:dropped]) \
            or sum(op != "D" for op in full) != len(dec_kept) or sum(op != "I" for op in full) != len(can_kept):
        raise ValueError("diagnose_indexed: the alignment path does not fit the phoneme counts")
    rows = []
    di, ci = dropped, 0                      # the dropped leading rows are insertions: decoded tokens only
    for op in d["path"]:
        i = c = None
        if op != "D":
            i = dec_kept[di]
            di += 1
        if op != "I":
            c = can_kept[ci]
            ci += 1
        rows.append((i, c))
    if di != len(dec_kept) or ci != len(can_kept):
        raise ValueError("diagnose_indexed: the alignment path does not fit the phoneme counts")
    return d, rows


def diagnose_timed(decoded_phones, spans, canonical_phones, canon_spans, decoder, seconds_per_frame, to_display=None):
    """``diagnose`` plus timing and goodness of pronunciation.  decoded_phones / canonical_phones: the phoneme strings ``diagnose``
    takes (or token lists); spans / canon_spans: one ``(start_frame, end_frame, mean_logp)`` per token of each, from the forced
    alignment of the decoded and of the canonical ids to the posteriors (``decode_timed`` / ``ctcDecoder.timed_spans``), or ``None``
    when that alignment is infeasible.  Returns ``diagnose``'s dict (computed by ``diagnose`` itself) with two more keys, both
    index-aligned with ``path``:
      times  (start_s, end_s, confidence = exp(mean_logp)) of the decoded phoneme on '-', 'S' and 'I' rows, None on 'D' rows (and on
             every row when ``spans`` is None).  Times are nominal frame starts, frame index x seconds_per_frame: the offset of the
             analysis window's centre is ignored.
      gop    the mean log-posterior of the canonical phoneme over its segment of the canonical alignment on '-', 'S' and 'D' rows,
             None on 'I' rows (and on every row when ``canon_spans`` is None).
    The spans follow their tokens through the 'sil' strip, the 'err' removal and the leading-insertion drops of ``diagnose`` /
    ``align_canonical_decoded``; a count that does not fit raises ValueError rather than mis-assigning a span."""
    dec, can = _tokens(decoded_phones), _tokens(canonical_phones)
    if spans is not None and len(spans) != len(dec):
        raise ValueError("diagnose_timed: %d spans for %d decoded phonemes" % (len(spans), len(dec)))
    if canon_spans is not None and len(canon_spans) != len(can):
        raise ValueError("diagnose_timed: %d spans for %d canonical phonemes" % (len(canon_spans), len(can)))
    d, rows = diagnose_indexed(dec, can, decoder, to_display)
    times, gop = [], []
    for i, c in rows:
        t = g = None
        if i is not None and spans is not None:
            s, e, m = spans[i]
            t = (s * seconds_per_frame, e * seconds_per_frame, math.exp(m))
        if c is not None and canon_spans is not None:
            g = canon_spans[c][2]
        times.append(t); gop.append(g)
    return dict(d, times=times, gop=gop)


def timed_lines(d):
    """The two extra lines of a printed block: ``time   : ph[start-end confidence] ...`` over the decoded row without its 'D'
    placeholders, ``gop    : ph[mean log-posterior] ...`` over the canonical row without its 'I' placeholders ('-' where unknown)."""
    tl = ["%s[%s]" % (p, "-" if t is None else "%.2f-%.2f %.2f" % t) for p, t, op in zip(d["decoded"], d["times"], d["path"]) if op != "D"]
    gl = ["%s[%s]" % (p, "-" if g is None else "%.2f" % g) for p, g, op in zip(d["canonical"], d["gop"], d["path"]) if op != "I"]
    return "time   : " + " ".join(tl), "gop    : " + " ".join(gl)


def diagnose_posterior(decoded_phones, canonical_phones, positions, decoder, names=None, to_display=None):
    """``diagnose`` plus the per-phoneme posteriors of the canonical sequence.  positions: one ``(p_correct, p_deleted, alt_id, p_alt)``
    per token of canonical_phones (the first element of an utterance's ``ctcDecoder.phoneme_posteriors`` result), or ``None`` when the
    canonical ids have no alignment.  Returns ``diagnose``'s dict with one more key, index-aligned with ``path``:
      post   (p_correct, p_deleted, alt, p_alt) of the canonical phoneme on '-', 'S' and 'D' rows -- alt is ``names[alt_id]`` when
             ``names`` (index -> phoneme) is given, passed through ``to_display`` like the rows, else alt_id -- None on 'I' rows (and on
             every row when ``positions`` is None).
    The entries follow their canonical tokens through the 'sil' strip exactly as ``diagnose_timed`` carries ``canon_spans``
    (``diagnose_indexed`` serves both)."""
    can = _tokens(canonical_phones)
    if positions is not None and len(positions) != len(can):
        raise ValueError("diagnose_posterior: %d entries for %d canonical phonemes" % (len(positions), len(can)))
    d, rows = diagnose_indexed(decoded_phones, can, decoder, to_display)

    def named(p):
        if names is None:
            return p
        alt = names[p[2]]
        if to_display is not None:
            alt = to_display.get(alt.upper(), alt)
        return (p[0], p[1], alt, p[3])

    post = [None if c is None or positions is None else named(positions[c]) for _, c in rows]
    return dict(d, post=post)


def posterior_line(d, label="post   : "):
    """The extra line of a printed block: ``post   : ph[p_correct alt:p_alt] ...`` over the canonical row without its 'I' placeholders;
    alt is the most probable single alternative -- 'del' when that is the deletion of the phoneme, else the best substitute -- and '-'
    stands for an unknown entry.  ``label`` is the line's head (``jpost  : `` for the joint marginals of ``joint_posteriors``)."""
    toks = []
    for p, q, op in zip(d["canonical"], d["post"], d["path"]):
        if op == "I":
            continue
        if q is None:
            toks.append("%s[-]" % p)
        else:
            alt, pa = ("del", q[1]) if q[1] >= q[3] else (q[2], q[3])
            toks.append("%s[%.2f %s:%.2f]" % (p, q[0], alt, pa))
    return label + " ".join(toks)


def _joint_name(k, names, to_display=None):
    ph = names[k]
    return to_display.get(ph.upper(), ph) if to_display is not None else ph


def joint_diagnosis_line(diag, ids, names, blank=0, to_display=None):
    """The ``jdiag  :`` line of a block from one utterance's ``ctcDecoder.joint_diagnosis`` result ``(positions, gaps, score,
    posterior)`` over the canonical ``ids``: ``jdiag  : <tokens> | edits <n> | score <%.4f> | p <%.4f>``.  The tokens run over the canonical
    ids (``names[id]``, passed through ``to_display`` as the other lines' are) with the gaps interleaved: ``ph`` kept, ``ph>alt``
    substituted by alt, ``ph>-`` deleted, ``+ph`` inserted; edits counts the tokens that are not plain.  ``jdiag  : -`` where the utterance
    has no result (``diag`` is None)."""
    if diag is None:
        return "jdiag  : -"
    positions, gaps, score, posterior = diag
    if len(positions) != len(ids) or len(gaps) != len(ids) + 1:
        raise ValueError("joint_diagnosis_line: %d positions and %d gaps for %d canonical phonemes" % (len(positions), len(gaps), len(ids)))
    toks, edits = [], 0
    for i in range(len(ids) + 1):
        if gaps[i][0] != blank:
            toks.append("+" + _joint_name(gaps[i][0], names, to_display))
            edits += 1
        if i == len(ids):
            break
        own, k = int(ids[i]), positions[i][0]
        ph = _joint_name(own, names, to_display)
        if k == own:
            toks.append(ph)
        else:
            toks.append(ph + ">" + ("-" if k == blank else _joint_name(k, names, to_display)))
            edits += 1
    return "jdiag  : %s | edits %d | score %.4f | p %.4f" % (" ".join(toks), edits, score, posterior)


def joint_time_line(diag, names, seconds_per_frame, blank=0, to_display=None):
    """The ``jtime  :`` line behind ``jdiag  :`` with ``timestamps``: ``jtime  : <ph> <start>-<end> ...`` over the labels the best reading
    emits, in slot order, in seconds as ``time   :`` prints them (nominal frame starts); ``jtime  : -`` where the utterance has no result."""
    if diag is None:
        return "jtime  : -"
    positions, gaps = diag[0], diag[1]
    toks = []
    for i in range(len(gaps)):
        for k, s, e in (gaps[i],) + ((positions[i],) if i < len(positions) else ()):
            if k != blank:
                toks.append("%s %.2f-%.2f" % (_joint_name(k, names, to_display), s * seconds_per_frame, e * seconds_per_frame))
    return "jtime  : " + " ".join(toks)


def seconds_per_frame(test_loader, cnn_time_stride):
    """Seconds between posterior frames: the fbank's frame shift x the loader's ``n_skip_frame`` x the CNN's time stride (0.04 s in
    the reference configuration)."""
    from .utils.fbank import FRAME_SHIFT_SAMPLES, SAMPLE_RATE
    skip = getattr(test_loader, "n_skip_frame", None)
    if skip is None:
        skip = getattr(getattr(test_loader, "dataset", None), "n_skip_frame", None)
    if skip is None:
        raise ValueError("timestamps need the loader's n_skip_frame (WavBatchLoader / SpeechDataLoader have it)")
    return FRAME_SHIFT_SAMPLES / float(SAMPLE_RATE) * int(skip) * int(cnn_time_stride)


def choose_pronunciation(loglik, count):
    """Index of the highest of the first ``count`` log-likelihoods; ties go to the earlier dictionary entry."""
    best = 0
    for p in range(1, count):
        if loglik[p] > loglik[best]:
            best = p
    return best


def pronunciation_line(phones, loglik, chosen):
    """The ``pron   :`` line of a block: every pronunciation with its CTC log-likelihood, the chosen one marked with '*'."""
    return "pron   : " + " | ".join("%s%s [%.4f]" % ("*" if p == chosen else "", ph, ll) for p, (ph, ll) in enumerate(zip(phones, loglik)))


def nbest_lines(records, canonical, decoder, to_display=None):
    """The ``nbest  :`` lines of a block, one per record ``(string, score, loglik, posterior)`` of ``BeamDecoder.decode_nbest``, best first:
    ``nbest  : <rank> <*|space> <phones> | score <beam score> | loglik <CTC log-likelihood> | p <share> | Comp. <correct>/<total>``.
    '*' marks rank 1, the hypothesis the block reports; score is the beam's length-normalised score, loglik the exact CTC log-likelihood
    ('-inf' for a hypothesis that is no CTC path), p its share among the listed hypotheses ('-' when none of them is a CTC path) and
    Comp. what ``diagnose`` counts for that hypothesis against the block's canonical ('-' where ``wer`` has nothing to align)."""
    lines = []
    for n, (hyp, score, loglik, share) in enumerate(records):
        try:
            d = diagnose(hyp, canonical, decoder, to_display)
            comp = "%d/%d" % (d["correct"], d["correct"] + d["del_sub"])
        except TypeError:                # an empty side after the 'sil' strip: Decoder.wer raises, as the reference's does
            comp = "-"
        lines.append("nbest  : %d %s %s | score %.4f | loglik %.4f | p %s | Comp. %s"
                     % (n + 1, "*" if n == 0 else " ", hyp, score, loglik, "-" if share is None else "%.4f" % share, comp))
    return lines


def mbr_line(record, canonical, decoder, to_display=None):
    """The ``mbr    :`` line of a block from one utterance's ``BeamDecoder.decode_mbr`` record ``(string, rank, risk, risk_of_rank_0,
    expected_errors_vs_canonical)``: ``mbr    : <rank> <phones> | risk <%.4f> | risk1 <%.4f> | exp <%.4f> | Comp. <correct>/<total>``.
    rank is the place of the minimum-Bayes-risk hypothesis in the N-best list, 1-based as ``nbest  :`` prints ranks; risk its expected
    number of phoneme errors against the list, risk1 the same for rank 1 (the block's decoded string), exp the list's expected edit
    distance to the block's canonical phones ('-' without them) and Comp. what ``diagnose`` counts for that hypothesis ('-' where
    ``wer`` has nothing to align).  ``mbr    : -`` where the utterance has no result (``record`` is None)."""
    if record is None:
        return "mbr    : -"
    hyp, rank, risk, risk1, exp = record
    try:
        d = diagnose(hyp, canonical, decoder, to_display)
        comp = "%d/%d" % (d["correct"], d["correct"] + d["del_sub"])
    except TypeError:                    # an empty side after the 'sil' strip: Decoder.wer raises, as the reference's does
        comp = "-"
    return "mbr    : %d %s | risk %.4f | risk1 %.4f | exp %s | Comp. %s" % (rank + 1, hyp, risk, risk1, "-" if exp is None else "%.4f" % exp, comp)


def infer(phonetic, word_dict, test_loader, device, model, decoder, vocab, test_transcipt_dict, use_ipa, out=None,
          decode_seq_path=None, timestamps=False, posteriors=False, pronunciations=False, nbest=0, joint_posteriors=False, error_prior=None,
          joint_diagnosis=False, mbr=0):
    """AA/infer.py:282-372.  Per batch ``(inputs, input_sizes, _, _, trans, trans_sizes, utt_list)``: ``model(inputs, trans)``,
    frame counts ``(input_sizes * T').long()``, ``decoder.decode``, then per utterance the 'sil' strip, 'err' removal, ``wer``,
    alignment, fault lists and score (``diagnose``), printed as the reference's 13-line block to ``out`` (stdout by default).
    Returns (total_correct_cnt, total_cnt, total_insertion_cnt).

    Offline substitutions: line 3 prints ``word_dict[utt]['ipa']`` as given; line 4 is ``phonetic.api_word_translation(word)``
    when ``phonetic`` has it (the reference asks ECDICT), else empty.  ``use_ipa`` needs ``phonetic.cmu_to_ipa_wiki``.  The
    reference always writes '<utt> <decoded phones>' lines to decode_seq.txt in the input folder and main() deletes the file;
    here they are written only when ``decode_seq_path`` is given.

    ``timestamps=True`` (no reference counterpart) adds two lines to each block between ``score  :`` and the closing empty line --
    ``time   :`` and ``gop    :`` (``diagnose_timed`` / ``timed_lines``) -- from two forced alignments per batch on the GPU: of the
    decoder's own ids and of the canonical ids.  Times are nominal frame starts (``seconds_per_frame``); nothing else changes.

    ``posteriors=True`` (no reference counterpart) adds one line, ``post   :`` (``diagnose_posterior`` / ``posterior_line``), before the
    closing empty line and after the ``timestamps`` lines if both are asked for: per canonical phoneme the probability that it was
    pronounced and the most probable alternative, from one ``phoneme_posteriors`` call per batch.  Without it nothing changes.

    ``pronunciations=True`` (no reference counterpart) takes the loader's 8-tuples (``WavBatchLoader(pronunciations=True)``): the batch's K
    candidate sets go through ``model.forward_candidates`` -- one acoustic pass, K conditioned posteriors -- and per utterance each distinct
    pronunciation is scored by the CTC log-likelihood of its own ids under its own posteriors (``hip_model.ctc_variants``' base over the
    utterance's frames; not length-normalised).  The highest wins, ties to the earlier dictionary entry, and the utterance's whole block --
    dictionary line, decode, alignment, diagnosis, score and the ``time`` / ``gop`` / ``post`` lines -- is that candidate's; a
    ``pron   :`` line (``pronunciation_line``) closes the block.  Without it nothing changes.

    ``nbest=N`` (no reference counterpart; needs a ``BeamDecoder`` with ``beam_width >= N >= 1``) adds N ``nbest  :`` lines
    (``nbest_lines``) before the closing empty line, after the ``time`` / ``gop`` / ``post`` lines and before ``pron``: the N best final
    hypotheses of the beam search (``decode_nbest``: the reference computes this list and keeps its head), each with its beam score, its
    exact CTC log-likelihood, its share of probability among the N and its ``Comp.`` against the block's canonical.  Rank 1 is the
    block's decoded string.  With ``pronunciations`` the lines are the chosen candidate's.  With 0 nothing changes.

    ``joint_posteriors=True`` (no reference counterpart) adds one line, ``jpost  :``, in the format of ``post   :`` and directly behind it
    (in front of ``nbest`` / ``pron``): the same per-phoneme figures as marginals over the whole error network of the canonical
    sequence -- every position kept, substituted or deleted and every gap empty or filled AT ONCE, not one edit with the rest taken as
    canonical (``ctcDecoder.joint_phoneme_posteriors``, one call per batch).  ``error_prior`` (0 < P < 1) is the prior probability of an
    error per slot; ``None`` weights every entry of every slot alike.  It reads only the posteriors, so it serves both model classes;
    with ``pronunciations`` the line is the chosen candidate's.  Without it nothing changes.

    ``joint_diagnosis=True`` (no reference counterpart; needs ``error_prior``, which it shares with ``joint_posteriors``) adds one line,
    ``jdiag  :`` (``joint_diagnosis_line``), directly behind ``jpost`` / ``post`` and in front of ``nbest`` / ``pron``: the single most
    probable combination of kept, substituted, deleted and inserted phonemes -- the best reading of the same error network with its
    alignment (``ctcDecoder.joint_diagnosis``, one call per batch) -- with its number of edits, its score and its probability among all
    readings.  With ``timestamps`` a ``jtime  :`` line (``joint_time_line``) follows it: the frames of every emitted phoneme in seconds.
    It reads only the posteriors, so it serves both model classes; with ``pronunciations`` the lines are the chosen candidate's.
    Without it nothing changes.

    ``mbr=N`` (no reference counterpart; needs a ``BeamDecoder`` with ``beam_width >= N >= 2``; independent of ``nbest``) adds one line,
    ``mbr    :`` (``mbr_line``), behind the ``nbest`` lines and in front of ``pron``: the minimum-Bayes-risk hypothesis of the N best --
    the one with the least expected edit distance to the list under the list's own CTC posterior (``decode_mbr``, one call per batch) --
    with its rank, its expected number of phoneme errors, the same figure for the block's decoded string and the list's expected edit
    distance to the canonical phones.  The block's decoded string, alignment and diagnosis stay the 1-best's.  It reads only the
    posteriors, so it serves both model classes; with ``pronunciations`` the line is the chosen candidate's.  With 0 nothing changes."""
    if error_prior is not None and not ((joint_posteriors or joint_diagnosis) and 0.0 < error_prior < 1.0):
        raise ValueError("error_prior needs joint_posteriors or joint_diagnosis and 0 < error_prior < 1")
    if joint_diagnosis and error_prior is None:
        raise ValueError("joint_diagnosis needs error_prior")
    if nbest and not (hasattr(decoder, "decode_nbest") and 1 <= nbest <= decoder.beam_width):
        raise ValueError("nbest needs a BeamDecoder and 1 <= nbest <= beam_width")
    if mbr and not (hasattr(decoder, "decode_mbr") and 2 <= mbr <= decoder.beam_width):
        raise ValueError("mbr needs a BeamDecoder and 2 <= mbr <= beam_width")
    if posteriors:
        from .utils.ctcDecoder import phoneme_posteriors
    if joint_posteriors:
        from .utils.ctcDecoder import joint_phoneme_posteriors
    if joint_diagnosis:
        from .utils.ctcDecoder import joint_diagnosis as joint_diagnosis_of
    if pronunciations:
        from .hip_model import ctc_variants
    out = sys.stdout if out is None else out
    to_display = phonetic.cmu_to_ipa_wiki if use_ipa else None
    translate = getattr(phonetic, "api_word_translation", None)
    total_correct_cnt = total_cnt = total_insertion_cnt = 0
    w1 = open(decode_seq_path, "w+") if decode_seq_path else None
    try:
        with torch.no_grad():
            for data in test_loader:
                inputs, input_sizes, _, _, trans, trans_sizes, utt_list = data[:7]
                inputs = inputs.to(device)
                # one (posteriors, canonical ids, lengths) per candidate set; without --pronunciations the batch itself
                if pronunciations:
                    sets = [(t.to(device), s) for t, s in data[7]["sets"]]
                    sets = [(p,) + ts for p, ts in zip(model.forward_candidates(inputs, [t for t, _ in sets]), sets)]
                else:
                    trans = trans.to(device)
                    sets = [(model(inputs, trans), trans, trans_sizes)]
                lens = frames_from_fraction(input_sizes, sets[0][0].size(0))
                frame_lens = lens.numpy().tolist()
                per_set = []     # what the blocks need of each set
                for probs, trans, trans_sizes in sets:
                    r = {}
                    if timestamps:
                        from .utils.ctcDecoder import timed_spans
                        r["decoded"], r["spans"] = decoder.decode_timed(probs, frame_lens)
                        r["canon_spans"] = timed_spans(probs, frame_lens, trans, trans_sizes, decoder.blank_index)
                        spf = seconds_per_frame(test_loader, inputs.size(1) // probs.size(0))
                    else:
                        r["decoded"] = decoder.decode(probs, frame_lens)
                    if nbest:
                        r["nbest"] = decoder.decode_nbest(probs, frame_lens, nbest)
                    if mbr:
                        r["mbr"] = decoder.decode_mbr(probs, frame_lens, mbr, trans, trans_sizes)
                    if posteriors:
                        r["post"] = phoneme_posteriors(probs, frame_lens, trans, trans_sizes, decoder.blank_index)
                    if joint_posteriors:
                        r["jpost"] = joint_phoneme_posteriors(probs, frame_lens, trans, trans_sizes, decoder.blank_index, error_prior)
                    if joint_diagnosis:
                        r["jdiag"] = joint_diagnosis_of(probs, frame_lens, trans, trans_sizes, decoder.blank_index, error_prior=error_prior)
                    if pronunciations:
                        r["loglik"] = ctc_variants(probs, frame_lens, trans.to(torch.int32), trans_sizes.to(torch.int32), decoder.blank_index,
                                                   want_ins=False).base.cpu().tolist()
                    r["trans"], r["trans_sizes"] = trans.cpu().numpy(), trans_sizes.numpy()
                    per_set.append(r)
                for x in range(len(utt_list)):
                    chosen = 0
                    if pronunciations:
                        count = data[7]["counts"][x]
                        loglik = [per_set[p]["loglik"][x] for p in range(count)]
                        chosen = choose_pronunciation(loglik, count)
                    r = per_set[chosen]
                    decoded, trans, trans_sizes = r["decoded"], r["trans"], r["trans_sizes"]
                    canonical = " ".join(vocab.index2word[num] for num in trans[x][:trans_sizes[x]])
                    utterance = test_transcipt_dict[utt_list[x]]
                    if timestamps:
                        d = diagnose_timed(decoded[x], r["spans"][x], canonical, r["canon_spans"][x], decoder, spf, to_display)
                    else:
                        d = diagnose(decoded[x], canonical, decoder, to_display)
                    tmp1, tmp2, tmp3 = d["printed"]
                    dict_line = word_dict[utt_list[x]]["cmu_all"][chosen] if pronunciations else word_dict[utt_list[x]]["ipa"]
                    block = ["id     : " + utt_list[x], utt_list[x] + ": " + utterance, str(dict_line),
                             str(translate(utterance)) if translate is not None else "", tmp2, tmp3, tmp1,
                             "ins err: " + " ".join(d["insertions"]), "sub err: " + " ".join(d["substitutions"]),
                             "del err: " + " ".join(d["deletions"]),
                             "Comp.  : " + str(d["correct"]) + "/" + str(d["correct"] + d["del_sub"]),
                             "score  : " + str(d["score"]), ""]
                    if timestamps:
                        block[-1:-1] = timed_lines(d)
                    if posteriors:
                        post = r["post"]
                        dp = diagnose_posterior(decoded[x], canonical, None if post[x] is None else post[x][0], decoder, vocab.index2word,
                                                to_display)
                        block[-1:-1] = [posterior_line(dp)]
                    if joint_posteriors:
                        post = r["jpost"]
                        dp = diagnose_posterior(decoded[x], canonical, None if post[x] is None else post[x][0], decoder, vocab.index2word,
                                                to_display)
                        block[-1:-1] = [posterior_line(dp, "jpost  : ")]
                    if joint_diagnosis:
                        own = trans[x][:trans_sizes[x]]
                        block[-1:-1] = [joint_diagnosis_line(r["jdiag"][x], own, vocab.index2word, decoder.blank_index, to_display)]
                        if timestamps:
                            block[-1:-1] = [joint_time_line(r["jdiag"][x], vocab.index2word, spf, decoder.blank_index, to_display)]
                    if nbest:
                        block[-1:-1] = nbest_lines(r["nbest"][x], canonical, decoder, to_display)
                    if mbr:
                        block[-1:-1] = [mbr_line(r["mbr"][x], canonical, decoder, to_display)]
                    if pronunciations:
                        phones = [" ".join(vocab.index2word[num] for num in per_set[p]["trans"][x][:per_set[p]["trans_sizes"][x]]) for p in range(count)]
                        block[-1:-1] = [pronunciation_line(phones, loglik, chosen)]
                    out.write("\n".join(block) + "\n")
                    total_correct_cnt += d["correct"]
                    total_cnt += d["correct"] + d["del_sub"]
                    total_insertion_cnt += len(d["insertions"])
                    if w1 is not None:
                        w1.write(utt_list[x] + " " + " ".join(d["decoded"]) + "\n")
    finally:
        if w1 is not None:
            w1.close()
    return total_correct_cnt, total_cnt, total_insertion_cnt
