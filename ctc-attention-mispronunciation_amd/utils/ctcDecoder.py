"""Drop-in for the reference's ``utils/ctcDecoder.py`` (AA/utils/ctcDecoder.py).

``GreedyDecoder`` / ``BeamDecoder`` keep the reference's constructor arguments and
``decode(prob_tensor, frame_seq_len) -> list[str]`` contract (same strings, same exception types);
the scans run in gfx950 kernels (mdd_greedy / mdd_beam, csrc/greedy.hip and csrc/beam.hip).  ``Decoder.wer`` keeps the
``(distance, op-path)`` return and runs the integer DP + backtrace natively on the host (mdd_align).
Posteriors may live on the GPU (no copy) or on the CPU as the reference passes them (copied in).
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .NgramLM import LanguageModel

_OPS = ("-", "S", "I", "D")
_BEAM_ERRORS = {1: IndexError("tuple index out of range"), 2: ValueError("math domain error"), 3: KeyError}


class Decoder(object):
    """String conversion and error metrics shared by both decoders (ctcDecoder.py:9-184)."""

    def __init__(self, int2char, space_idx=1, blank_index=0):
        self.int_to_char = int2char
        self.space_idx = space_idx
        self.blank_index = blank_index
        self.num_word = 0
        self.num_char = 0

    def decode(self):
        raise NotImplementedError

    # -- string helpers (ctcDecoder.py:80-116)
    def _convert_to_string(self, seq, sizes):
        chars = [self.int_to_char[seq[i]] for i in range(sizes)]
        return chars if self.space_idx == -1 else "".join(chars)

    def _convert_to_strings(self, seq, sizes=None):
        return [self._convert_to_string(seq[x], sizes[x] if sizes is not None else len(seq[x])) for x in range(len(seq))]

    def _process_string(self, seq, remove_rep=False):
        out = ""
        blank = self.int_to_char[self.blank_index]
        for i, ch in enumerate(seq):
            if ch == blank or (remove_rep and i != 0 and ch == seq[i - 1]):
                continue
            if self.space_idx == -1:
                out += " " + ch
            elif ch == self.int_to_char[self.space_idx]:
                out += " "
            else:
                out += ch
        return out

    def _process_strings(self, seqs, remove_rep=False):
        return [self._process_string(s, remove_rep) for s in seqs]

    def _unflatten_targets(self, targets, target_sizes):
        out, off = [], 0
        for size in target_sizes:
            out.append(targets[off:off + size])
            off += size
        return out

    # -- metrics (ctcDecoder.py:118-184)
    def _edit_distance(self, src_seq, tgt_seq):
        """Reference quirk kept: a bare int (not a tuple) when either side is empty (ctcDecoder.py:137-138)."""
        if len(src_seq) == 0:
            return len(tgt_seq)
        if len(tgt_seq) == 0:
            return len(src_seq)
        dist, ops = align_ids(_tokens_to_ids(src_seq, tgt_seq))
        return dist, ops

    def wer(self, s1, s2):
        """Word-level edit distance of two space-separated strings and its op path
        ('-' match, 'S' substitution, 'I' token only in s1, 'D' token only in s2)."""
        ans, paths = self._edit_distance(s1.split(), s2.split())   # TypeError on an empty side, like the reference
        return ans, paths

    def cer(self, s1, s2):
        ans, _ = self._edit_distance(s1, s2)
        return ans

    def phone_word_error(self, prob_tensor, frame_seq_len, targets, target_sizes):
        strings = self.decode(prob_tensor, frame_seq_len)
        refs = self._process_strings(self._convert_to_strings(self._unflatten_targets(targets, target_sizes)))
        cer = wer = 0
        for hyp, ref in zip(strings, refs):
            cer += self.cer(hyp, ref)
            wer += self.wer(hyp, ref)[0]
            self.num_word += len(ref.split())
            self.num_char += len(ref)
        return cer, wer


def _tokens_to_ids(a, b):
    table = {}
    ia = [table.setdefault(t, len(table)) for t in a]
    ib = [table.setdefault(t, len(table)) for t in b]
    return ia, ib


def align_ids(pair):
    """(dist, ops) for two non-empty integer sequences via the native mdd_align."""
    a = np.ascontiguousarray(pair[0], dtype=np.int32)
    b = np.ascontiguousarray(pair[1], dtype=np.int32)
    ops = np.zeros(len(a) + len(b) + 1, dtype=np.uint8)
    dist, nops = C.c_int32(0), C.c_int32(0)
    _lib.check(_lib.lib().mdd_align(_lib.ptr(a), len(a), _lib.ptr(b), len(b), C.byref(dist), _lib.ptr(ops), C.byref(nops)))
    return dist.value, [_OPS[o] for o in ops[:nops.value]]


def align_ids_batch(a, a_len, b, b_len):
    """Edit distance and op path of every row pair of two padded id matrices in one native call (mdd_align_batch).

    a [n, Sa], b [n, Sb] int32 with per-row lengths; returns (dist [n], ops [n, Sa+Sb] uint8 codes 0 '-', 1 'S', 2 'I',
    3 'D', nops [n]).  A row with an empty side has dist -1 and no ops (the reference's ``wer`` raises there)."""
    a = np.ascontiguousarray(a, dtype=np.int32); b = np.ascontiguousarray(b, dtype=np.int32)
    a_len = np.ascontiguousarray(a_len, dtype=np.int32); b_len = np.ascontiguousarray(b_len, dtype=np.int32)
    if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0] or a_len.shape != (a.shape[0],) or b_len.shape != (a.shape[0],):
        raise ValueError("align_ids_batch: a [n, Sa], b [n, Sb], a_len [n], b_len [n]")
    n, stride = a.shape[0], a.shape[1] + b.shape[1]
    dist, nops = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    ops = np.zeros((n, max(stride, 1)), dtype=np.uint8)
    p = _lib.ptr
    _lib.check(_lib.lib().mdd_align_batch(p(a), p(a_len), a.shape[1], p(b), p(b_len), b.shape[1], n, p(dist), p(ops), ops.shape[1], p(nops)))
    return dist, ops, nops


def _device_posteriors(prob_tensor):
    _lib.require_gpu()
    if prob_tensor.dim() != 3:
        raise ValueError("prob_tensor must be [T, B, C]")
    return _lib.to_gpu(prob_tensor, torch.float32)


def _lens_tensor(frame_seq_len, B, T, dev):
    if frame_seq_len is None:
        frame_seq_len = [T] * B
    if torch.is_tensor(frame_seq_len):
        return frame_seq_len.to(dev, torch.int32).contiguous()
    return torch.tensor([int(v) for v in frame_seq_len], dtype=torch.int32, device=dev)


def _posteriors_and_lens(prob_tensor, frame_seq_len):
    """(lp, T, B, C, lens): the posteriors on their device and the int32 frame counts beside them."""
    lp = _device_posteriors(prob_tensor)
    T, B, Cn = lp.shape
    return lp, T, B, Cn, _lens_tensor(frame_seq_len, B, T, lp.device)


def _pick_tuples(pos_rows, gap_rows, own_ids, blank):
    """``phoneme_posteriors``' ``(positions, gaps)`` from rows of probabilities: pos_rows[i] over the C entries of position i (own id,
    blank = deleted, substitutes), gap_rows[g] over those of gap g (blank = nothing inserted, insertions)."""
    positions, gaps = [], []
    for p, own in zip(pos_rows, own_ids):
        own = int(own)
        alt = p.copy()
        alt[own] = alt[blank] = -1.0
        k = int(alt.argmax())
        positions.append((float(p[own]), float(p[blank]), k, float(p[k])))
    for p in gap_rows:
        alt = p.copy()
        alt[blank] = -1.0
        k = int(alt.argmax())
        gaps.append((k, float(p[k])))
    return positions, gaps


def timed_spans(prob_tensor, frame_seq_len, ids, nids, blank=0):
    """Forced alignment of ``ids`` / ``nids`` ([B, stride] / [B], as ``decode_ids`` returns them) to the posteriors (mdd_ctc_align):
    per utterance a list of ``(start_frame, end_frame, mean_logp)``, one per id -- the first frame, one past the last frame and the mean
    log-posterior of the id over its frames -- or ``None`` when the ids have no feasible alignment (or are no valid targets)."""
    from ..hip_model import ctc_align
    lp, T, B, _, lens = _posteriors_and_lens(prob_tensor, frame_seq_len)
    r = ctc_align(lp, lens, ids, nids, blank=blank, want_path=False)
    status, seg, seg_logp, n = r.status.cpu().numpy(), r.seg.cpu().numpy(), r.seg_logp.cpu().numpy(), torch.as_tensor(nids).cpu().numpy()
    out = []
    for b in range(B):
        if status[b] != 0:
            out.append(None)
            continue
        out.append([(int(seg[b, i, 0]), int(seg[b, i, 1]), float(seg_logp[b, i]) / int(seg[b, i, 1] - seg[b, i, 0])) for i in range(int(n[b]))])
    return out


def phoneme_posteriors(prob_tensor, frame_seq_len, ids, nids, blank=0):
    """Per-phoneme posteriors of the canonical ``ids`` / ``nids`` ([B, stride] / [B]) from the CTC likelihood of every sequence one edit
    away (mdd_ctc_variants).  Per utterance ``None`` when the ids are no valid targets or have no alignment themselves, else
    ``(positions, gaps)``: positions[i] = ``(p_correct, p_deleted, alt_id, p_alt)`` -- the softmax over the C entries of sub[b, i, :]
    (the phoneme itself, its deletion, each substitute), alt_id the most probable substitute and p_alt its probability; gaps[g] =
    ``(ins_id, p_ins)`` for 0 <= g <= nids[b] -- the most probable insertion before position g in the softmax over ins[b, g, :], whose
    blank entry is "nothing inserted".  Variants without an alignment have probability 0."""
    from ..hip_model import ctc_variants
    lp, T, B, _, lens = _posteriors_and_lens(prob_tensor, frame_seq_len)
    ids_h, n = torch.as_tensor(ids).cpu().numpy(), torch.as_tensor(nids).cpu().numpy()
    r = ctc_variants(lp, lens, ids, nids, blank=blank, max_len=min(max(int(n.max()), 0), ids_h.shape[1]))     # no slots past the longest row
    status, sub, ins = r.status.cpu().numpy(), r.sub.cpu().numpy(), r.ins.cpu().numpy()

    def softmax(row):
        with np.errstate(under="ignore"):
            e = np.exp(row - row.max())      # -inf entries: exactly 0
        return e / e.sum()

    out = []
    for b in range(B):
        if status[b] != 0:
            out.append(None)
            continue
        L = int(n[b])
        out.append(_pick_tuples([softmax(sub[b, i]) for i in range(L)], [softmax(ins[b, g]) for g in range(L + 1)], ids_h[b, :L], blank))
    return out


def error_network(ids, nids, num_class, blank=0, error_prior=None):
    """The error network of the canonical ``ids`` / ``nids`` ([B, stride] / [B]) for ``hip_model.ctc_confnet``: ``(w [B, 2 stride + 1,
    C] float32, nslots = 2 nids + 1)``.  Slot 2g is the gap before position g (entry blank: nothing inserted, entry k: k inserted), slot
    2i + 1 is position i (entry ids[i]: the phoneme itself, entry blank: deleted, entry k: substituted by k).  ``error_prior=None``: every
    entry of every slot has log-weight 0 -- the uniform prior ``phoneme_posteriors`` implies, under which a gap offers C - 1 insertions
    at the weight of "nothing".  ``error_prior=P`` (0 < P < 1): a position keeps its phoneme with log(1 - P) and every other entry gets
    log(P / (C - 1)); a gap stays empty with log(1 - P) and every insertion gets log(P / (C - 1)).  Rows at or past 2 nids + 1 are
    filled like gaps and never read."""
    import math
    ids = torch.as_tensor(ids)
    nids = torch.as_tensor(nids)
    if ids.dim() != 2 or nids.shape != (ids.shape[0],):
        raise ValueError("error_network: ids [B, stride], nids [B]")
    if error_prior is not None and not 0.0 < error_prior < 1.0:
        raise ValueError("error_network: 0 < error_prior < 1")
    if not 0 <= blank < num_class or num_class < 2:
        raise ValueError("error_network: blank outside [0, num_class)")
    B, stride = ids.shape
    dev = ids.device
    keep, err = (0.0, 0.0) if error_prior is None else (math.log1p(-error_prior), math.log(error_prior / (num_class - 1)))
    w = torch.full((B, 2 * stride + 1, num_class), err, dtype=torch.float32, device=dev)
    w[:, 0::2, blank] = keep
    if stride:
        own = ids.to(torch.int64).clamp(0, num_class - 1).unsqueeze(2)         # an id outside [0, C) is refused by nids / status, not here
        w[:, 1::2, :].scatter_(2, own, keep)
    return w, (2 * nids.to(torch.int32) + 1)


def _posterior_tuples(post, total, status, ids_h, n, blank):
    """``phoneme_posteriors``' result from the marginals of an error network: post [B, >= 2 n + 1, C], total [B] (log values)."""
    out = []
    for b in range(len(n)):
        if status[b] != 0:
            out.append(None)
            continue
        with np.errstate(under="ignore"):
            p_all = np.exp(post[b] - total[b])         # -inf entries: exactly 0
        L = int(n[b])
        out.append(_pick_tuples(p_all[1:2 * L:2], p_all[0:2 * L + 1:2], ids_h[b, :L], blank))
    return out


def joint_phoneme_posteriors(prob_tensor, frame_seq_len, ids, nids, blank=0, error_prior=None):
    """``phoneme_posteriors``' result -- per utterance ``None`` or ``(positions, gaps)`` with the same tuples -- where every number is a
    marginal over the whole error network of ``ids`` (``error_network``, mdd_ctc_confnet): all positions may be kept, substituted or
    deleted and all gaps filled in the same reading, each reading weighted by its entries' priors and the CTC likelihood of what it
    emits.  ``None``: ids that are no valid targets, or a network without any alignment."""
    from ..hip_model import ctc_confnet
    lp, T, B, Cn, lens = _posteriors_and_lens(prob_tensor, frame_seq_len)
    ids_h, n = torch.as_tensor(ids).cpu().numpy(), torch.as_tensor(nids).cpu().numpy()
    valid = [0 <= int(n[b]) <= ids_h.shape[1] and all(0 <= int(v) < Cn and int(v) != blank for v in ids_h[b, :max(int(n[b]), 0)])
             for b in range(B)]
    Lmax = min(max(int(n.max()), 0), ids_h.shape[1]) if B else 0           # no slots past the longest row
    w, nslots = error_network(torch.as_tensor(ids)[:, :Lmax], torch.as_tensor(nids), Cn, blank, error_prior)
    nslots = torch.where(torch.as_tensor(valid), nslots.cpu(), torch.full((B,), -1, dtype=torch.int32))       # not a target: BAD_TARGET
    r = ctc_confnet(lp, lens, w, nslots, blank=blank)
    return _posterior_tuples(r.post.cpu().numpy(), r.total.cpu().numpy(), r.status.cpu().numpy(), ids_h, n, blank)


def joint_diagnosis(prob_tensor, frame_seq_len, ids, nids, blank=0, *, error_prior):
    """The single most probable combination of kept, substituted, deleted and inserted phonemes of the canonical ``ids`` / ``nids``
    ([B, stride] / [B]) with the frames each phoneme occupies: the best reading of ``error_network(ids, error_prior)`` and its alignment
    (mdd_ctc_confnet_best).  ``error_prior`` is required, 0 < P < 1: under the uniform prior a substitution ties exactly with a deletion
    plus an insertion, and the tie rule alone would decide.  Per utterance ``None`` (ids that are no valid targets, or a network without
    any alignment) or ``(positions, gaps, score, posterior)``:
      positions[i] = (entry, start, end)   entry ids[i]: kept, ``blank``: deleted, else the substitute; the frames [start, end) of what
                                           was emitted, -1, -1 for a deletion
      gaps[g]      = (entry, start, end)   for 0 <= g <= nids[b]; ``blank``: nothing inserted before position g
      score        the reading's weights plus the log-posteriors of its best path (float64)
      posterior    exp(sum_j w[j, r_j] + log P_CTC(labels) - total): the reading's probability among all readings of the network, over
                   all of its alignments (one ``ctc_variants`` base on the reading's labels, one ``ctc_confnet`` total), float64."""
    from ..hip_model import ctc_confnet, ctc_confnet_best, ctc_variants
    if error_prior is None or not 0.0 < error_prior < 1.0:
        raise ValueError("joint_diagnosis: 0 < error_prior < 1")
    lp, T, B, Cn, lens = _posteriors_and_lens(prob_tensor, frame_seq_len)
    ids_h, n = torch.as_tensor(ids).cpu().numpy(), torch.as_tensor(nids).cpu().numpy()
    valid = [0 <= int(n[b]) <= ids_h.shape[1] and all(0 <= int(v) < Cn and int(v) != blank for v in ids_h[b, :max(int(n[b]), 0)])
             for b in range(B)]
    Lmax = min(max(int(n.max()), 0), ids_h.shape[1]) if B else 0           # no slots past the longest row
    w, nslots = error_network(torch.as_tensor(ids)[:, :Lmax], torch.as_tensor(nids), Cn, blank, error_prior)
    nslots = torch.where(torch.as_tensor(valid), nslots.cpu(), torch.full((B,), -1, dtype=torch.int32))       # not a target: BAD_TARGET
    r = ctc_confnet_best(lp, lens, w, nslots, blank=blank, want_path=False)
    total = ctc_confnet(lp, lens, w, nslots, blank=blank, want_post=False).total.cpu().numpy()
    status, reading, seg, score = r.status.cpu().numpy(), r.reading.cpu().numpy(), r.seg.cpu().numpy(), r.score.cpu().numpy()
    w_h = w.cpu().numpy().astype(np.float64)
    # log P_CTC of each reading's labels: one base per utterance
    labels = [[int(k) for k in reading[b, :2 * int(n[b]) + 1] if k != blank] if status[b] == 0 else [] for b in range(B)]
    lab = np.full((B, max(1, max((len(v) for v in labels), default=0))), 1 if blank == 0 else 0, dtype=np.int32)   # padding: a label, never read
    for b, v in enumerate(labels):
        lab[b, :len(v)] = v
    base = ctc_variants(lp, lens, torch.from_numpy(lab), torch.tensor([len(v) for v in labels], dtype=torch.int32), blank=blank,
                        want_ins=False).base.cpu().numpy()
    out = []
    for b in range(B):
        if status[b] != 0:
            out.append(None)
            continue
        L = int(n[b])
        slots = [(int(reading[b, j]), int(seg[b, j, 0]), int(seg[b, j, 1])) for j in range(2 * L + 1)]
        prior = float(sum(w_h[b, j, k] for j, (k, _, _) in enumerate(slots)))
        out.append((slots[1::2], slots[0::2], float(score[b]), float(np.exp(prior + float(base[b]) - float(total[b])))))
    return out


def nbest_posteriors(loglik):
    """Float64 softmax over one utterance's N log-likelihoods: the share of probability each listed hypothesis holds AMONG THE LISTED
    ONES, not an absolute probability (what the list leaves out is not counted).  ``-inf`` entries get 0; ``None`` when every entry
    is ``-inf`` (no listed hypothesis is a CTC path of the posteriors)."""
    ll = np.asarray(loglik, dtype=np.float64).reshape(-1)
    top = ll.max() if ll.size else -np.inf
    if not top > -np.inf:
        return None
    with np.errstate(under="ignore"):
        e = np.exp(ll - top)             # -inf entries: exactly 0
    return e / e.sum()


class GreedyDecoder(Decoder):
    """argmax per frame, collapse repeats, drop blanks (ctcDecoder.py:186-200)."""

    def decode_ids(self, prob_tensor, frame_seq_len=None):
        lp, T, B, Cn, lens = _posteriors_and_lens(prob_tensor, frame_seq_len)
        ids = torch.empty((B, T), dtype=torch.int32, device=lp.device)
        nids = torch.empty((B,), dtype=torch.int32, device=lp.device)
        p = _lib.ptr
        with torch.cuda.device(lp.device):
            _lib.check(_lib.lib().mdd_greedy(p(lp), T, B, Cn, p(lens), self.blank_index, p(ids), p(nids), _lib.current_stream_ptr()))
        return ids, nids

    def decode(self, prob_tensor, frame_seq_len):
        return self._strings(*self.decode_ids(prob_tensor, frame_seq_len))

    def decode_timed(self, prob_tensor, frame_seq_len):
        """``decode`` plus, per utterance, the ``(start_frame, end_frame, mean_logp)`` of every decoded id (``timed_spans`` on the
        decoder's own ids: the alignment of the greedy ids is the per-frame argmax path)."""
        lp = _device_posteriors(prob_tensor)
        ids, nids = self.decode_ids(lp, frame_seq_len)
        return self._strings(ids, nids), timed_spans(lp, frame_seq_len, ids, nids, self.blank_index)

    def _strings(self, ids, nids):
        ids, nids = ids.cpu().numpy(), nids.cpu().numpy()
        out = []
        for b in range(ids.shape[0]):
            chars = [self.int_to_char[int(i)] for i in ids[b, :nids[b]]]
            if self.space_idx == -1:
                out.append("".join(" " + c for c in chars))
            else:
                sp = self.int_to_char[self.space_idx]
                out.append("".join(" " if c == sp else c for c in chars))
        return out


class BeamDecoder(Decoder):
    """CTC prefix beam search with a bigram LM hook (ctcDecoder.py:202-226, BeamSearch.py:73-153)."""

    def __init__(self, int2char, beam_width=200, blank_index=0, space_idx=-1, lm_path=None, lm_alpha=0.01):
        self.beam_width = beam_width
        super(BeamDecoder, self).__init__(int2char, space_idx=space_idx, blank_index=blank_index)
        self.lm = LanguageModel(arpa_file=lm_path)
        self.lm_alpha = lm_alpha
        self._tables = {}

    def _lm_table(self, num_class, dev):
        key = (num_class, str(dev))
        if key not in self._tables:
            self._tables[key] = torch.from_numpy(self.lm.dense_table(self.int_to_char, num_class)).to(dev)
        return self._tables[key]

    def _search(self, entry, prob_tensor, frame_seq_len, N, *nbest):
        """mdd_beam (``nbest`` empty, N = 1) or mdd_beam_nbest (``nbest`` = (N,)): (ids [N,B,T], nids [N,B], status [B], score [N,B]).
        A shape those two refuse on size (mdd_beam_fits: beam_width over 64, or state past their LDS limits) goes to mdd_beam_wide with the
        same N, which has their outputs and takes beam_width up to 256 at any length; it refuses what is left by its own message."""
        lp, T, B, Cn, lens = _posteriors_and_lens(prob_tensor, frame_seq_len)
        ids = torch.empty((N, B, T), dtype=torch.int32, device=lp.device)
        nids = torch.empty((N, B), dtype=torch.int32, device=lp.device)
        status = torch.empty((B,), dtype=torch.int32, device=lp.device)
        score = torch.empty((N, B), dtype=torch.float64, device=lp.device)
        lm, p = self._lm_table(Cn, lp.device), _lib.ptr
        with torch.cuda.device(lp.device):
            if _lib.lib().mdd_beam_fits(T, B, Cn, self.beam_width):
                _lib.check(entry(p(lp), T, B, Cn, p(lens), self.beam_width, self.blank_index, p(lm), float(self.lm_alpha), *nbest,
                                 p(ids), p(nids), p(status), p(score), _lib.current_stream_ptr()))
            else:
                _lib.check(_lib.lib().mdd_beam_wide(p(lp), T, B, Cn, p(lens), self.beam_width, self.blank_index, p(lm), float(self.lm_alpha), N,
                                                    p(ids), p(nids), p(status), p(score), None, 0, _lib.current_stream_ptr()))
        return ids, nids, status, score

    def decode_ids(self, prob_tensor, frame_seq_len=None):
        ids, nids, status, score = self._search(_lib.lib().mdd_beam, prob_tensor, frame_seq_len, 1)
        return ids[0], nids[0], status, score[0]

    def decode(self, prob_tensor, frame_seq_len=None):
        ids, nids, status, _ = self.decode_ids(prob_tensor, frame_seq_len)
        return self._strings(ids, nids, status)

    def decode_timed(self, prob_tensor, frame_seq_len=None):
        """``decode`` (same strings, same exceptions first) plus, per utterance, the ``(start_frame, end_frame, mean_logp)`` of every
        decoded id, or ``None`` for an utterance whose winner has no feasible alignment: the beam skips near-certain blank frames and
        merges repeats by its own rule, so its winner need not be a CTC path of the posteriors."""
        lp = _device_posteriors(prob_tensor)
        ids, nids, status, _ = self.decode_ids(lp, frame_seq_len)
        strings = self._strings(ids, nids, status)
        return strings, timed_spans(lp, frame_seq_len, ids, nids, self.blank_index)

    def decode_nbest_ids(self, prob_tensor, frame_seq_len=None, nbest=None):
        """The ``nbest`` (default ``beam_width``) best final hypotheses of every utterance (mdd_beam_nbest), as device tensors
        ``(ids [N,B,T], nids [N,B], status [B], score [N,B])``: slice n is ``decode_ids``' output for the hypothesis of rank n, slice 0
        its output itself, bit for bit.  Ranks follow the reference's final sort: descending length-normalised score, equal scores in
        the order of the final beam.  An utterance with an error status has nids 0 and score NaN in every slice.  Nothing synchronises."""
        N = self.beam_width if nbest is None else int(nbest)
        if not 1 <= N <= self.beam_width:
            raise ValueError("nbest must be in [1, beam_width = %d]" % self.beam_width)
        return self._search(_lib.lib().mdd_beam_nbest, prob_tensor, frame_seq_len, N, N)

    def nbest_loglik(self, prob_tensor, frame_seq_len, ids, nids, max_len=None):
        """Exact CTC log-likelihood of every hypothesis of ``decode_nbest_ids``' ``ids [N,B,T]`` / ``nids [N,B]`` over its utterance's
        frames, as a float64 numpy array [N,B]: the fp32 nll of the training lattice, negated, ``-inf`` where the lattice finds no path.
        ``max_len`` bounds nids (default: the ids' row length); a tight bound lets the lattice keep fewer labels per lane.  Where
        ``hip_model.ctc_nbest_fits`` takes the shape, all ranks are one ``hip_model.ctc_nbest`` launch, rounded through fp32 as the nll
        is; otherwise (hypotheses past 255 ids, posteriors past the launch's LDS bound) one ``hip_model.ctc_loss`` call without
        gradient per slice.  The same bytes either way."""
        from .. import hip_model
        lp, T, B, Cn, lens = _posteriors_and_lens(prob_tensor, frame_seq_len)
        lens = lens.clamp(0, T)
        width = ids.shape[2] if max_len is None else max(min(int(max_len), ids.shape[2]), 1)
        if 1 <= ids.shape[0] <= 256 and hip_model.ctc_nbest_fits(T, Cn, width):
            loglik = hip_model.ctc_nbest(lp, lens, ids, nids, blank=self.blank_index, max_len=min(width, ids.shape[2]))
            return -(-loglik).float().double().cpu().numpy()
        nll = [hip_model.ctc_loss(lp, ids[n, :, :width], lens, nids[n], blank=self.blank_index, want_grad=False)[0] for n in range(ids.shape[0])]
        return -torch.stack(nll).double().cpu().numpy()

    def decode_nbest(self, prob_tensor, frame_seq_len=None, nbest=None, rescore=True):
        """Per utterance a list of N records ``(string, score, loglik, posterior)``, best first; record 0's string is ``decode``'s
        string and the exceptions are ``decode``'s.  ``score`` is the beam's own length-normalised score, which is no CTC likelihood
        (the search skips near-certain blank frames and applies its repeat rule to raw frames).  ``rescore`` adds ``loglik``, the exact
        CTC log-likelihood of the hypothesis over the utterance's frames (``nbest_loglik``; ``-inf`` for a hypothesis that is no CTC path
        of the posteriors), and ``posterior``, its share among the N listed hypotheses
        (``nbest_posteriors``: relative to the list, not an absolute probability; ``None`` when no hypothesis of the list is a CTC
        path).  With ``rescore=False`` both are ``None``."""
        lp, T, B, _, lens = _posteriors_and_lens(prob_tensor, frame_seq_len)
        ids, nids, status, score = self.decode_nbest_ids(lp, lens, nbest)
        N = ids.shape[0]
        nids_h = nids.cpu().numpy()
        strings = [self._strings(ids[n], nids_h[n], status) for n in range(N)]      # raises decode's exception
        loglik = self.nbest_loglik(lp, lens, ids, nids, max_len=int(nids_h.max())) if rescore else None
        score_h = score.cpu().numpy()
        out = []
        for b in range(B):
            post = nbest_posteriors(loglik[:, b]) if rescore else None
            out.append([(strings[n][b], float(score_h[n, b]), float(loglik[n, b]) if rescore else None,
                         None if post is None else float(post[n])) for n in range(N)])
        return out

    def decode_mbr(self, prob_tensor, frame_seq_len=None, nbest=None, canonical_ids=None, canonical_lens=None):
        """The minimum-Bayes-risk ("consensus") hypothesis of the N-best list: among the ``nbest`` (default ``beam_width``) final
        hypotheses the one with the least expected edit distance to the others, each weighted by its share of the list's exact CTC
        likelihood -- ``decode_nbest_ids`` -> ``nbest_loglik`` -> ``nbest_posteriors`` -> ``hip_model.nbest_mbr`` (mdd_nbest_mbr).  The
        phoneme error rate is an edit distance, so this is the listed hypothesis that minimises the expected number of phoneme errors
        under the list's own posterior; ties go to the better rank, so a list that agrees with itself keeps ``decode``'s answer.
        Per utterance ``(string, rank, risk, risk_of_rank_0, expected_errors_vs_canonical | None)``: the hypothesis and its place in the
        list (0 is ``decode``'s string), its expected number of phoneme errors against the list, the same figure for rank 0, and --
        with ``canonical_ids`` [B, L] / ``canonical_lens`` [B] -- the list's expected edit distance to the canonical phones.  ``None``
        for an utterance the kernel flags: no listed hypothesis is a CTC path of the posteriors (all weights 0), or an id is outside
        the classes.  The exceptions are ``decode``'s; a hypothesis or canonical row longer than 1024 ids raises ``ValueError``."""
        from ..hip_model import MBR_MAX_LEN, nbest_mbr
        lp, T, B, Cn, lens = _posteriors_and_lens(prob_tensor, frame_seq_len)
        ids, nids, status, _ = self.decode_nbest_ids(lp, lens, nbest)
        N = ids.shape[0]
        self._strings(ids[0], nids[0], status)                      # rank 0 as decode builds it: raises decode's exception
        ids_h, nids_h = ids.cpu().numpy(), nids.cpu().numpy()      # one download of the list; a string is built for the chosen rank alone
        longest = int(nids_h.max())
        ref = ref_len = None
        if canonical_ids is not None:
            ref, ref_len = torch.as_tensor(canonical_ids), torch.as_tensor(canonical_lens)
            longest = max(longest, int(ref_len.max()) if ref_len.numel() else 0)
        if longest > MBR_MAX_LEN:
            raise ValueError("decode_mbr: a sequence of %d ids; mdd_nbest_mbr takes at most %d" % (longest, MBR_MAX_LEN))
        mbr_ids = ids
        if longest > ids.shape[2]:       # a canonical row longer than the T frames a hypothesis row holds: max_len bounds both, so widen the rows
            mbr_ids = torch.nn.functional.pad(ids, (0, longest - ids.shape[2]))
        loglik = self.nbest_loglik(lp, lens, ids, nids, max_len=int(nids_h.max()))
        weights = np.zeros((N, B), dtype=np.float64)
        for b in range(B):
            post = nbest_posteriors(loglik[:, b])
            if post is not None:
                weights[:, b] = post
        best, risk, flag, _, _, ref_risk = nbest_mbr(mbr_ids, nids, status, torch.from_numpy(weights), Cn, max_len=max(longest, 1), ref=ref,
                                                     ref_len=ref_len)
        best, risk, flag = best.cpu().numpy(), risk.cpu().numpy(), flag.cpu().numpy()
        ref_risk = None if ref_risk is None else ref_risk.cpu().numpy()
        out = []
        for b in range(B):
            if flag[b] != 0:
                out.append(None)
                continue
            k = int(best[b])
            string = " ".join(self.int_to_char[int(i)] for i in ids_h[k, b, :nids_h[k, b]])
            out.append((string, k, float(risk[k, b]), float(risk[0, b]), None if ref_risk is None else float(ref_risk[b])))
        return out

    def _strings(self, ids, nids, status):
        ids, nids, status = ids.cpu().numpy(), torch.as_tensor(nids).cpu().numpy(), status.cpu().numpy()
        bad = np.nonzero(status)[0]
        if len(bad):   # the reference stops at the first utterance that raises
            err = _BEAM_ERRORS[int(status[bad[0]])]
            raise err("utterance %d of the batch" % bad[0]) if err is KeyError else err
        return [" ".join(self.int_to_char[int(i)] for i in ids[b, :nids[b]]) for b in range(ids.shape[0])]
