"""The yardstick of the N-best beam ending -- TEST INFRASTRUCTURE, CPU only.

``nbest`` is the project's pure-Python prefix beam (oracle/ref_port.beam: a dict of prefix tuple -> [total, nonblank, blank] with the
reference's rules) restated so that it returns what the reference's ending computes before it takes ``[0]`` (AA/utils/BeamSearch.py:
130-148): the final state, EOS-scored and length-normalised, in ``sorted(..., reverse=True)`` order -- descending score, equal scores
in the order of ``BHat`` (Python's sort is stable and the final state is filled in BHat order).  Pinned to the reference itself by
tests/golden/g16_nbest.* (tools/gen_golden_nbest.py), and to oracle.beam's winner on every decoder case (tests/test_nbest_reference.py).

The language model is the dense table the C ABI takes (NaN = KeyError).  ``exp`` chooses how log-posteriors become the fp32
probabilities the search works on: "torch" is torch.exp in fp32 (the reference, ctcDecoder.py:224), "f64" a float64 exp rounded once
to fp32 (what the GPU pre-pass computes).  The two differ by one ulp on about 1 % of the inputs; a test case must rank alike under both.
"""
import functools
import math

import numpy as np
import torch

LOG_ZERO = -99999999.0
STATUS = {IndexError: 1, ValueError: 2, KeyError: 3}      # include/mdd_hip.h: mdd_beam_status
EXP_FLAVOURS = ("torch", "f64")


def probabilities(logp, exp):
    """[T, B, C] float32 log-posteriors -> [B, T, C] float32 probabilities."""
    lp = np.array(logp, dtype=np.float32)             # a copy: the shared inputs are read-only
    if exp == "torch":
        p = torch.exp(torch.from_numpy(lp)).numpy()
    elif exp == "f64":
        with np.errstate(under="ignore"):
            p = np.exp(lp.astype(np.float64)).astype(np.float32)
    else:
        raise ValueError(exp)
    return np.ascontiguousarray(p.transpose(1, 0, 2))


def _ladd(a, b):
    if a <= LOG_ZERO:
        return b
    if b <= LOG_ZERO:
        return a
    if b - a > 0.0:
        a, b = b, a
    return a + math.log(1 + math.exp(b - a))


def _lm(table, prev, nxt):
    v = table[prev, nxt]
    if v != v:
        raise KeyError((prev, nxt))
    return float(v)


def final_list(mat, n_frames, table, beam_width, alpha, blank):
    """One utterance: mat [T, C] float32 probabilities -> the whole ranked final list [(ids, score)]; raises what the reference raises."""
    C = mat.shape[1]
    last = {(): [0.0, LOG_ZERO, 0.0]}
    for t in range(n_frames):
        if (1 - mat[t, blank]) < 0.1:
            continue
        keep = sorted(last.items(), key=lambda kv: kv[1][0], reverse=True)[:beam_width]
        curr = {}
        for y, (tot, nb, bl) in keep:
            p_nb = nb + math.log(mat[t, y[-1]]) if y else LOG_ZERO
            p_bl = tot + math.log(mat[t, blank])
            e = curr.setdefault(y, [LOG_ZERO, LOG_ZERO, LOG_ZERO])
            e[1] = _ladd(e[1], p_nb)
            e[2] = _ladd(e[2], p_bl)
            e[0] = _ladd(e[0], _ladd(p_bl, p_nb))
            for k in range(C):
                if k == blank:
                    continue
                big = _lm(table, y[-1] if y else C, k) * alpha
                base = bl if (y and y[-1] == k and mat[t - 1, blank] < 0.9) else tot
                pr = math.log(mat[t, k]) + big + base
                e2 = curr.setdefault(y + (k,), [LOG_ZERO, LOG_ZERO, LOG_ZERO])
                e2[1] = _ladd(e2[1], pr)
                e2[0] = _ladd(e2[0], pr)
        last = curr
    keep = sorted(last.items(), key=lambda kv: kv[1][0], reverse=True)[:beam_width]
    final = []
    for y, (tot, nb, bl) in keep:
        pr = _ladd(LOG_ZERO, tot + _lm(table, y[-1], C) * alpha)          # IndexError on the empty prefix
        final.append((pr * (1.0 / (len(y) if len(y) else 1)), y))
    ranked = sorted(final, key=lambda v: v[0], reverse=True)              # stable: equal scores stay in BHat order
    # a status-0 utterance always ends with exactly `beam` hypotheses: every kept prefix re-enters the next state as itself, and while
    # the state holds fewer the empty prefix is still among them (IndexError above).  The ABI has no count output because of this.
    assert len(ranked) == beam_width, (len(ranked), beam_width)
    return [(list(y), s) for s, y in ranked]


def nbest(logp, lens, table, beam_width=10, alpha=0.0, blank=0, exp="torch", rows=None):
    """logp [T, B, C], lens [B], table [(C+1), (C+1)] float64 -> per utterance of ``rows`` (default: all) ``(final, status)``: the ranked
    list [(ids, score)] and 0, or [] and the mdd_beam_status code of the exception the reference raises."""
    T = logp.shape[0]
    probs = probabilities(logp, exp)
    table = np.asarray(table, dtype=np.float64)
    out = []
    for b in (range(probs.shape[0]) if rows is None else rows):
        try:
            out.append((final_list(probs[b], max(0, min(int(lens[b]), T)), table, beam_width, alpha, blank), 0))
        except (IndexError, ValueError, KeyError) as e:
            out.append(([], STATUS[type(e)]))
    return out


# ------------------------------------------------------------------------------------------- the decoder cases (tests/test_decoders.py)
def spread_rows(B, k):
    """The rows of a batch of B the yardstick decodes when a case allows k of them (None: all): spread over the batch with distinct
    b % 12, so that every wave position of a workgroup packed with 2, 3 or 4 utterances is hit (and every row kind of the `errors`
    family, which go by b % 12), plus the last row, which sits in the last, partly empty workgroup."""
    if k is None or k >= B:
        return tuple(range(B))
    residues = (0, 1, 2, 7, 3, 4, 5, 6, 8, 9, 10, 11)[:k]
    rows = {12 * ((i * ((B - 1 - r) // 12)) // max(len(residues) - 1, 1)) + r for i, r in enumerate(residues)}
    rows.add(B - 1)
    assert all(0 <= b < B for b in rows)
    return tuple(sorted(rows))


@functools.lru_cache(maxsize=None)
def case_lists(case, exp="torch"):
    """(rows, [(final, status)]) of a test_decoders case, computed once per flavour and shared; an utterance whose probabilities are
    the same bits under both flavours is decoded once."""
    from tests.test_decoders import inputs
    logp, lens, lm = inputs(case)
    rows = spread_rows(case.B, case.port_rows)
    if exp == "torch":
        return rows, nbest(logp, lens, lm, case.beam, case.alpha, case.blank, "torch", rows)
    _, base = case_lists(case, "torch")
    pa, pb = probabilities(logp, "torch"), probabilities(logp, exp)
    n = [max(0, min(int(lens[b]), case.T)) for b in rows]
    same = [np.array_equal(pa[b, :n[i]], pb[b, :n[i]]) for i, b in enumerate(rows)]
    fresh = iter(nbest(logp, lens, lm, case.beam, case.alpha, case.blank, exp, [b for i, b in enumerate(rows) if not same[i]]))
    return rows, [base[i] if same[i] else next(fresh) for i in range(len(rows))]
