"""One-edit CTC variants (mdd_ctc_variants, csrc/ctc_variants.hip) against a float64 brute force.

Reference (``brute``): every variant's own target through CPU ``torch.nn.functional.ctc_loss`` in double, ``reduction='none'``; the empty
target is the sum of the blank's log-posteriors.  ``formula_variants`` restates DESIGN.md "One-edit variants" in float64 numpy: it is
checked against the brute force on the CPU, so a GPU failure can be told apart from a wrong formula.

Numeric bound (finite entries, absolute): BOUND = 4 x the largest error measured over ``all_cases()`` on an MI355X by
tools/ctc_variants_margins.py (profiles/ctc_variants_margins.json: 8.2e-7 over 11,259 finite entries, beside 7.6e-6 for mdd_ctc_loss's fp32
nll on the same inputs), the factor 4 for input-dependent rounding, and never past the project's 1e-4 log-prob tolerance.  -inf
positions must be the reference's exactly."""
import ctypes as C
import functools
import io
import os
import types

import numpy as np
import pytest

NEG = -np.inf
OK, INFEASIBLE, BAD = 0, 1, 2
SENTINEL = 12345.0
CAP = 1e-4
MEASURED_MAX = 8.17e-7      # profiles/ctc_variants_margins.json "variants_max_abs_err", rounded up
BOUND = min(4 * MEASURED_MAX, CAP)


# ------------------------------------------------------------------------------------------------------------ the references
def variant_target(y, blank, kind, pos, k):
    """The label list of one variant: ('s', i, k) substitution (k == blank: deletion, k == y[i]: y itself), ('i', g, k) insertion
    (k == blank: y itself)."""
    y = list(y)
    if kind == "s":
        return y[:pos] + ([] if k == blank else [k]) + y[pos + 1:]
    return y[:pos] + ([] if k == blank else [k]) + y[pos:]


def brute(lp, Tb, targets, blank):
    """log P(target) for every target; lp [T, C] (any float dtype, used as float64), the first Tb frames count."""
    import torch
    import torch.nn.functional as F
    out = np.full(len(targets), NEG)
    if Tb == 0:
        for n, tg in enumerate(targets):
            if not tg:
                out[n] = 0.0
        return out
    lp = np.asarray(lp[:Tb], dtype=np.float64)
    full = [n for n, tg in enumerate(targets) if tg]
    for n, tg in enumerate(targets):
        if not tg:
            out[n] = lp[:, blank].sum()
    if full:
        Lm = max(len(targets[n]) for n in full)
        tgt = np.full((len(full), Lm), (blank + 1) % lp.shape[1], dtype=np.int64)
        for r, n in enumerate(full):
            tgt[r, :len(targets[n])] = targets[n]
        x = torch.from_numpy(lp).unsqueeze(1).expand(Tb, len(full), lp.shape[1]).contiguous()
        nll = F.ctc_loss(x, torch.from_numpy(tgt), torch.full((len(full),), Tb, dtype=torch.long),
                         torch.tensor([len(targets[n]) for n in full], dtype=torch.long), blank=blank, reduction="none")
        out[full] = -nll.numpy()
    assert not np.isnan(out).any() and not np.isposinf(out).any()
    return out


def _lattices(lp, y, blank):
    """alpha, beta [T, 2L+1] in float64, both including the emission at t."""
    T, L = lp.shape[0], len(y)
    S = 2 * L + 1
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = y
    skip = np.zeros(S, dtype=bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    al = np.full((T, S), NEG)
    be = np.full((T, S), NEG)
    al[0, 0] = lp[0, blank]
    if L:
        al[0, 1] = lp[0, y[0]]
    for t in range(1, T):
        for s in range(S):
            v = al[t - 1, s]
            if s >= 1:
                v = np.logaddexp(v, al[t - 1, s - 1])
            if skip[s]:
                v = np.logaddexp(v, al[t - 1, s - 2])
            al[t, s] = v + lp[t, ext[s]]
    be[T - 1, S - 1] = lp[T - 1, blank]
    if L:
        be[T - 1, S - 2] = lp[T - 1, y[-1]]
    for t in range(T - 2, -1, -1):
        for s in range(S):
            v = be[t + 1, s]
            if s + 1 < S:
                v = np.logaddexp(v, be[t + 1, s + 1])
            if s + 2 < S and skip[s + 2]:
                v = np.logaddexp(v, be[t + 1, s + 2])
            be[t, s] = v + lp[t, ext[s]]
    return al, be


def formula_variants(lp, Tb, y, blank):
    """DESIGN.md "One-edit variants" in float64: (base, sub [L, C], ins [L+1, C]) for Tb >= 1."""
    lp = np.asarray(lp[:Tb], dtype=np.float64)
    T, Cn, L = Tb, lp.shape[1], len(y)
    with np.errstate(invalid="ignore"):
        return _formula(lp, T, Cn, L, list(y), blank)


def _formula(lp, T, Cn, L, y, blank):
    lae = np.logaddexp
    al, be = _lattices(lp, y, blank)
    base = lae(al[T - 1, 2 * L], al[T - 1, 2 * L - 1] if L else NEG)

    def slot(sL, sR, k):
        left = y[sL // 2 - 1] if sL >= 1 else None
        right = y[(sR + 1) // 2] if sR + 1 <= 2 * L else None
        g, acc = NEG, NEG
        for t in range(T):
            if t == 0:
                i_t = 0.0 if sL == 0 else NEG
            else:
                i_t = al[t - 1, sL]
                if left is not None and left != k:
                    i_t = lae(i_t, al[t - 1, sL - 1])
            g = lae(g, i_t) + lp[t, k]
            if t == T - 1:
                o_t = 0.0 if sR == 2 * L else NEG
            else:
                o_t = be[t + 1, sR]
                if right is not None and right != k:
                    o_t = lae(o_t, be[t + 1, sR + 1])
            acc = lae(acc, g + o_t)
        return acc

    def deletion(i):
        skip = i >= 1 and i + 1 < L and y[i - 1] != y[i + 1]
        acc = NEG
        if i + 1 < L:
            for t in range(T - 1):
                a = al[t, 2 * i]
                if skip:
                    a = lae(a, al[t, 2 * i - 1])
                acc = lae(acc, a + be[t + 1, 2 * i + 3])
        if i == L - 1:
            acc = lae(acc, al[T - 1, 2 * i])
            if i >= 1:
                acc = lae(acc, al[T - 1, 2 * i - 1])
        if i == 0 and L > 1:
            acc = lae(acc, be[0, 3])
        return acc

    sub = np.full((L, Cn), NEG)
    ins = np.full((L + 1, Cn), NEG)
    for i in range(L):
        for k in range(Cn):
            sub[i, k] = deletion(i) if k == blank else (base if k == y[i] else slot(2 * i, 2 * i + 2, k))
    for g in range(L + 1):
        for k in range(Cn):
            ins[g, k] = base if k == blank else slot(2 * g, 2 * g, k)
    return base, sub, ins


def all_entries(L, Cn):
    return [("s", i, k) for i in range(L) for k in range(Cn)] + [("i", g, k) for g in range(L + 1) for k in range(Cn)]


def sampled_entries(L, Cn, blank, rs, n=300):
    """All deletions, and n substitutions and insertions drawn at random."""
    e = [("s", i, blank) for i in range(L)]
    for _ in range(n):
        if rs.integers(2):
            e.append(("s", int(rs.integers(L)), int(rs.integers(Cn))))
        else:
            e.append(("i", int(rs.integers(L + 1)), int(rs.integers(Cn))))
    return e


# ------------------------------------------------------------------------------------------------------------ CPU tests
def test_formulas_match_the_brute_force_in_float64():
    rs = np.random.default_rng(3)
    n_inf = n = 0
    for case in range(60):
        T, L, Cn = int(rs.integers(1, 8)), int(rs.integers(1, 5)), int(rs.integers(3, 6))
        blank = int(rs.integers(Cn))
        labels = [c for c in range(Cn) if c != blank]
        y = [labels[int(rs.integers(len(labels)))] for _ in range(L)]
        if L > 1 and case % 3 == 0:
            y[1] = y[0]
        lp = np.log(rs.dirichlet(np.ones(Cn), size=T))
        base, sub, ins = formula_variants(lp, T, y, blank)
        ent = all_entries(L, Cn)
        want = brute(lp, T, [variant_target(y, blank, *e) for e in ent], blank)
        got = np.array([(sub if kind == "s" else ins)[pos, k] for kind, pos, k in ent])
        assert (np.isneginf(got) == np.isneginf(want)).all(), (T, y, blank)
        fin = np.isfinite(want)
        assert np.abs(got[fin] - want[fin]).max(initial=0.0) < 1e-12, (T, y, blank)
        assert np.isneginf(base) == np.isneginf(brute(lp, T, [y], blank)[0])
        n += len(ent); n_inf += int((~fin).sum())
    assert n > 1000 and n_inf > 100       # both kinds of outcome are exercised


def _lib():
    from ctc_attention_mispronunciation_amd import _lib
    return _lib.lib()


def test_variants_rejects_bad_arguments_before_device_work():
    """Every argument error returns MDD_ERR_ARG and names the argument; host addresses stand in for device buffers, none is used."""
    L_ = _lib()
    host = np.zeros(64, np.float32)
    buf = C.c_void_p(host.ctypes.data)
    good = dict(logp=buf, T=10, B=2, C=5, len=buf, ids=buf, stride=8, nids=buf, Lmax=8, blank=0, base=buf, sub=buf, ins=buf, status=buf,
                ws=None, ws_bytes=0)
    order = ["logp", "T", "B", "C", "len", "ids", "stride", "nids", "Lmax", "blank", "base", "sub", "ins", "status", "ws", "ws_bytes"]
    need = L_.mdd_ctc_variants_workspace_bytes(10, 2, 5, 8)
    assert need >= 8 * 2 * 10 * 2 * 17 and L_.mdd_ctc_variants_workspace_bytes(400, 2, 5, 300) >= 8 * 2 * 400 * 2 * 601
    cases = [(dict(logp=None), "logp_dev"), (dict(len=None), "len_dev"), (dict(ids=None), "ids_dev"), (dict(nids=None), "nids_dev"),
             (dict(base=None), "base_dev"), (dict(sub=None), "sub_dev"), (dict(status=None), "status_dev"), (dict(T=0), "T"),
             (dict(B=0), "B"), (dict(C=0), "C"), (dict(T=-3), "T"), (dict(C=257, blank=0), "C > 256"), (dict(blank=-1), "blank"),
             (dict(blank=5), "blank"), (dict(Lmax=9), "Lmax"), (dict(Lmax=-1), "Lmax"), (dict(ws=buf, ws_bytes=need - 1), "workspace"),
             (dict(stride=6000, Lmax=6000), "Lmax too long")]       # past the wave form and past the general form's LDS rows
    for change, name in cases:
        a = dict(good, **change)
        assert L_.mdd_ctc_variants(*[a[k] for k in order], None) == -1, change
        assert name in L_.mdd_last_error().decode(), (change, L_.mdd_last_error().decode())


def test_ctc_loss_rejects_bad_arguments_before_device_work():
    """mdd_ctc_loss refuses as the entries built on its lattice do: MDD_ERR_ARG, the argument named, a caller workspace one byte short
    refused too; host addresses stand in for device buffers, none is used and no HIP call is reached (this runs without a GPU)."""
    L_ = _lib()
    host = np.zeros(64, np.float32)
    buf = C.c_void_p(host.ctypes.data)
    good = dict(logp=buf, T=10, B=2, C=5, targets=buf, Lmax=8, in_len=buf, tgt_len=buf, blank=0, nll=buf, grad=buf, ws=None, ws_bytes=0)
    order = ["logp", "T", "B", "C", "targets", "Lmax", "in_len", "tgt_len", "blank", "nll", "grad", "ws", "ws_bytes"]
    need = L_.mdd_ctc_workspace_bytes(10, 2, 5, 8, 1)
    assert need >= 8 * 2 * 10 * 17
    cases = [(dict(logp=None), "logp_dev"), (dict(targets=None), "targets_dev"), (dict(in_len=None), "in_len_dev"),
             (dict(tgt_len=None), "tgt_len_dev"), (dict(nll=None), "nll_dev"), (dict(T=0), "T <= 0"), (dict(B=0), "B <= 0"),
             (dict(C=0), "C <= 0"), (dict(T=-3), "T <= 0"), (dict(B=-1), "B <= 0"), (dict(C=-2), "C <= 0"), (dict(Lmax=-1), "Lmax < 0"),
             (dict(blank=-1), "blank outside"), (dict(blank=5), "blank outside"), (dict(ws=buf, ws_bytes=need - 1), "workspace")]
    for change, name in cases:
        a = dict(good, **change)
        assert L_.mdd_ctc_loss(*[a[k] for k in order], None) == -1, change
        msg = L_.mdd_last_error().decode()
        assert msg.startswith("mdd_ctc_loss: ") and name in msg, (change, msg)


def _decoder():
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import Decoder
    return Decoder({0: "blank"}, space_idx=-1, blank_index=0)


def test_diagnose_posterior_follows_the_canonical_tokens():
    from ctc_attention_mispronunciation_amd.infer_core import diagnose, diagnose_posterior
    names = {0: "blank", 1: "a", 2: "b", 3: "x"}
    post = lambda n: [(0.5 + i / 100.0, 0.1, 3, 0.2) for i in range(n)]      # noqa: E731   p_correct carries the token index
    # 'sil' at both ends of the canonical row is stripped with its entry; the middle has a substitution, a deletion and an insertion
    dec, can = "a x c e f q g", "sil a b c d e f g sil"
    d = diagnose_posterior(dec, can, post(9), _decoder(), names)
    base = diagnose(dec, can, _decoder())
    assert {k: d[k] for k in base} == base and set(d) == set(base) | {"post"}
    assert d["path"] == ["-", "S", "-", "D", "-", "-", "I", "-"]
    idx = [None if p is None else int(round((p[0] - 0.5) * 100)) for p in d["post"]]
    assert idx == [1, 2, 3, 4, 5, 6, None, 7]
    assert all(p is None or p[1:] == (0.1, "x", 0.2) for p in d["post"])
    # leading insertions are decoded tokens only; ids stay ids without a name table; display names apply to the alternative
    d = diagnose_posterior("x y z a b", "a b", post(2), _decoder())
    assert d["path"] == ["I", "-", "-"] and d["post"][0] is None and [p[2] for p in d["post"][1:]] == [3, 3]
    d = diagnose_posterior("a b", "a b", post(2), _decoder(), names, to_display={"X": "XX", "A": "AA"})
    assert d["canonical"] == ["AA", "b"] and [p[2] for p in d["post"]] == ["XX", "XX"]
    d = diagnose_posterior("a x c", "a b c", None, _decoder(), names)
    assert d["post"] == [None, None, None]
    with pytest.raises(ValueError, match="2 entries for 3 canonical"):
        diagnose_posterior("a b c", "a b c", post(2), _decoder(), names)


def test_posterior_line_format():
    from ctc_attention_mispronunciation_amd.infer_core import posterior_line
    d = dict(canonical=["ph", "b", "I", "c"], path=["-", "D", "I", "S"],
             post=[(0.934, 0.01, "ih", 0.04), (0.2, 0.7, "d", 0.05), None, (0.3, 0.25, "s", 0.25)])
    assert posterior_line(d) == "post   : ph[0.93 ih:0.04] b[0.20 del:0.70] c[0.30 del:0.25]"
    d["post"] = [None] * 4
    assert posterior_line(d) == "post   : ph[-] b[-] c[-]"


# ------------------------------------------------------------------------------------------------------------ the device call
def gpu_variants(lp, lens, ids, nids, Lmax, blank, ws="torch", want_ins=True):
    """mdd_ctc_variants through ctypes on sentinel-filled buffers.  ws: 'torch' (caller workspace of the stated size) or None (NULL)."""
    import torch
    L_ = _lib()
    T, B, Cn = lp.shape
    stride = ids.shape[1]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    lp_d, len_d, nid_d = d(lp.astype(np.float32)), d(np.asarray(lens, np.int32)), d(np.asarray(nids, np.int32))
    ids_d = d(ids.astype(np.int32)) if stride else torch.zeros(1, dtype=torch.int32, device="cuda")
    base = torch.full((B,), SENTINEL, dtype=torch.float64, device="cuda")
    sub = torch.full((B, max(stride, 1), Cn), SENTINEL, dtype=torch.float64, device="cuda")
    ins = torch.full((B, stride + 1, Cn), SENTINEL, dtype=torch.float64, device="cuda")
    status = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    need = L_.mdd_ctc_variants_workspace_bytes(T, B, Cn, Lmax)
    wsbuf = torch.empty(need, dtype=torch.uint8, device="cuda") if ws == "torch" else None
    rc = L_.mdd_ctc_variants(p(lp_d), T, B, Cn, p(len_d), p(ids_d), stride, p(nid_d), Lmax, blank, p(base), p(sub),
                             p(ins) if want_ins else None, p(status), p(wsbuf) if wsbuf is not None else None,
                             wsbuf.numel() if wsbuf is not None else 0, None)
    assert rc == 0, L_.mdd_last_error().decode()
    torch.cuda.synchronize()
    return dict(base=base.cpu().numpy(), sub=sub.cpu().numpy()[:, :stride], ins=ins.cpu().numpy(), status=status.cpu().numpy())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def compare(got, lp, lens, ids, nids, blank, entries):
    """Every listed entry of every utterance against the brute force: -inf where and only where the reference is, finite entries within
    BOUND; base and status likewise.  entries: per utterance a list of (kind, pos, k), or None for all.  Returns (max |error|, count)."""
    T, B, Cn = lp.shape
    worst, count = 0.0, 0
    for b in range(B):
        Tb, L = min(max(int(lens[b]), 0), T), int(nids[b])
        y = [int(v) for v in ids[b, :L]]
        ent = all_entries(L, Cn) if entries is None or entries[b] is None else entries[b]
        want = brute(lp[:, b, :], Tb, [y] + [variant_target(y, blank, *e) for e in ent], blank)
        have = np.array([got["base"][b]] + [(got["sub"] if kind == "s" else got["ins"])[b, pos, k] for kind, pos, k in ent])
        assert got["status"][b] == (INFEASIBLE if np.isneginf(want[0]) else OK), (b, got["status"][b], want[0])
        wrong = np.isneginf(have) != np.isneginf(want)
        assert not wrong.any(), (b, [([("base",)] + ent)[n] for n in np.nonzero(wrong)[0][:5]], have[wrong][:5], want[wrong][:5])
        fin = np.isfinite(want)
        assert np.isfinite(have[fin]).all(), b
        err = np.abs(have[fin] - want[fin])
        print("utterance %d: L %d, len %d, %d finite entries, max |error| %.3e" % (b, L, Tb, int(fin.sum()), err.max(initial=0.0)))
        worst, count = max(worst, float(err.max(initial=0.0))), count + int(fin.sum())
    return worst, count


def run_case(case):
    got = gpu_variants(case["lp"], case["lens"], case["ids"], case["nids"], case["Lmax"], case["blank"])
    worst, count = compare(got, case["lp"], case["lens"], case["ids"], case["nids"], case["blank"], case["entries"])
    return got, worst, count


def check_case(case):
    got, worst, _ = run_case(case)
    assert worst <= BOUND, (case["name"], worst, BOUND)
    return got


# ------------------------------------------------------------------------------------------------------------ the cases
def _posteriors(rs, T, B, Cn, scale=2.0):
    x = rs.standard_normal((T, B, Cn)) * scale
    x = x - np.log(np.exp(x).sum(axis=-1, keepdims=True))
    return x.astype(np.float32)


def _pack(rows, stride):
    ids = np.zeros((len(rows), stride), np.int32)
    for b, y in enumerate(rows):
        ids[b, :len(y)] = y
    return ids, np.array([len(y) for y in rows], np.int32)


def _labels(rs, L, classes, repeats=2):
    """L labels without adjacent repeats, then `repeats` positions made equal to their left neighbour."""
    y = []
    for _ in range(L):
        c = classes[int(rs.integers(len(classes)))]
        while y and c == y[-1]:
            c = classes[int(rs.integers(len(classes)))]
        y.append(c)
    for j in rs.choice(np.arange(1, L), size=min(repeats, L - 1), replace=False) if L > 1 else []:
        y[j] = y[j - 1]
    return y


def exhaustive_cases(blank):
    """T = 9, C = 6, B = 4 ragged, L in 1..4 with repeats at every place a repeat can sit; every entry of every row."""
    Cn, T = 6, 9
    a, b_, c, d = [k for k in range(Cn) if k != blank][:4]
    rows = [[a], [a, a], [a, b_], [a, b_, a], [a, a, b_], [a, b_, b_], [a, b_, c], [a, a, a], [a, b_, c, d], [a, b_, a, b_], [a, a, b_, b_],
            [a, b_, b_, a]]
    lens = [9, 7, 5, 3, 9, 4, 8, 6, 9, 7, 5, 6]
    rs = np.random.default_rng(100 + blank)
    for n in range(0, len(rows), 4):
        ids, nids = _pack(rows[n:n + 4], 5)
        yield dict(name="exhaustive blank %d batch %d" % (blank, n // 4), lp=_posteriors(rs, T, 4, Cn), lens=lens[n:n + 4], ids=ids, nids=nids,
                   Lmax=4, blank=blank, entries=None)


def lane_case(L):
    """Lmax = L at the edges of the lattice's labels-per-lane forms (63 | 64, 65 | 129) and, at 300, the general lattice kernel."""
    rs = np.random.default_rng(L)
    Cn, blank = 5, 0
    T = 330 if L == 300 else L + 8
    rows = [_labels(rs, L, [1, 2, 3, 4]), _labels(rs, L // 2, [1, 2, 3, 4])]
    ids, nids = _pack(rows, L)
    return dict(name="L %d" % L, lp=_posteriors(rs, T, 2, Cn), lens=[T, T - 5], ids=ids, nids=nids, Lmax=L, blank=blank,
                entries=[sampled_entries(L, Cn, blank, rs), sampled_entries(L // 2, Cn, blank, rs, 100)])


def lds_case():
    """T = 713, C = 45, L = 12: the general lattice kernel reached through the LDS rule of csrc/ctc.hip (713 frames of 45 log-probs beside the
    wave kernel's lists are 12 bytes past its 128 KB; T = 712 is the last wave shape), not through the label count as L = 300 does.  Held to
    BOUND as it stands and kept out of ``all_cases``, which BOUND was measured over; measured on an MI355X: 1.24e-6 over 171 finite entries
    (the error grows with the frame count: 8.2e-7 was the worst at T <= 330)."""
    rs = np.random.default_rng(713)
    T, Cn, L, blank = 713, 45, 12, 0
    classes = list(range(1, Cn))
    rows = [_labels(rs, L, classes), _labels(rs, 7, classes)]
    ids, nids = _pack(rows, L)
    return dict(name="T 713 by the LDS rule", lp=_posteriors(rs, T, 2, Cn), lens=[T, T - 60], ids=ids, nids=nids, Lmax=L, blank=blank,
                entries=[sampled_entries(L, Cn, blank, rs, 100), sampled_entries(7, Cn, blank, rs, 50)])


def class_case(Cn, blank):
    rs = np.random.default_rng(1000 * Cn + blank)
    labels = [k for k in range(Cn) if k != blank]
    rows = [[labels[0], labels[-1], labels[len(labels) // 2]], [labels[-1], labels[-1], labels[1]]]
    ids, nids = _pack(rows, 3)
    return dict(name="C %d blank %d" % (Cn, blank), lp=_posteriors(rs, 12, 2, Cn), lens=[12, 9], ids=ids, nids=nids, Lmax=3, blank=blank,
                entries=None)


def edge_cases():
    rs = np.random.default_rng(77)
    Cn, blank = 4, 1
    rows = [[0], [0, 2], [2, 2], [], [3, 0]]
    for T in (1, 2):
        ids, nids = _pack(rows, 3)
        yield dict(name="T %d" % T, lp=_posteriors(rs, T, 5, Cn), lens=[T] * 5, ids=ids, nids=nids, Lmax=2, blank=blank, entries=None)
    # no frames at all, next to utterances that have some: the empty variant scores 0, every other -inf
    ids, nids = _pack([[0], [], [0, 2], [2], [3, 0, 2]], 3)
    yield dict(name="len 0", lp=_posteriors(rs, 6, 5, Cn), lens=[0, 0, 0, 6, 0], ids=ids, nids=nids, Lmax=3, blank=blank, entries=None)
    # frames >= len are never read: NaN there must not reach any output
    lp = _posteriors(rs, 10, 3, Cn)
    lens = [4, 10, 7]
    for b, n in enumerate(lens):
        lp[n:, b, :] = np.nan
    ids, nids = _pack([[0, 2], [2, 0, 3], [3, 3]], 3)
    yield dict(name="NaN past len", lp=lp, lens=lens, ids=ids, nids=nids, Lmax=3, blank=blank, entries=None)
    # whole classes the model rules out: -inf in every frame (a canonical label among them, and the blank in one utterance)
    lp = _posteriors(rs, 8, 3, 5)
    lp[:, 0, 2] = NEG
    lp[:, 1, 3] = NEG; lp[:, 1, 4] = NEG
    lp[:, 2, 1] = NEG
    ids, nids = _pack([[0, 2, 3], [0, 2], [4, 0]], 3)
    yield dict(name="classes at -inf", lp=lp, lens=[8, 8, 6], ids=ids, nids=nids, Lmax=3, blank=1, entries=None)


LANE_L = (63, 64, 65, 129, 300)
CLASS_CASES = [(Cn, bl) for Cn in (45, 64, 65, 70) for bl in (Cn - 1, Cn // 2)]


def all_cases():
    """Every case the bound is measured over (tools/ctc_variants_margins.py)."""
    for blank in (0, 3, 5):
        yield from exhaustive_cases(blank)
    for L in LANE_L:
        yield lane_case(L)
    for Cn, bl in CLASS_CASES:
        yield class_case(Cn, bl)
    yield from edge_cases()


# ------------------------------------------------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("blank", (0, 3, 5))
def test_exhaustive_small(blank):
    for case in exhaustive_cases(blank):
        check_case(case)


@pytest.mark.gpu
@pytest.mark.parametrize("L", LANE_L)
def test_lattice_lane_ownership_and_general_lattice(L):
    check_case(lane_case(L))


@pytest.mark.gpu
def test_general_lattice_through_the_lds_rule():
    case = lds_case()
    T, B, Cn = case["lp"].shape
    assert _lib().mdd_ctc_variants_workspace_bytes(T, B, Cn, case["Lmax"]) == 8 * 2 * B * T * (2 * case["Lmax"] + 1)      # the general form's rows
    assert _lib().mdd_ctc_variants_workspace_bytes(T - 1, B, Cn, case["Lmax"]) == 16 * B * (T - 1) * 2 * (case["Lmax"] + 1)
    check_case(case)


@pytest.mark.gpu
@pytest.mark.parametrize("Cn,blank", CLASS_CASES)
def test_class_loop_and_blank_position(Cn, blank):
    check_case(class_case(Cn, blank))


@pytest.mark.gpu
def test_edges():
    for case in edge_cases():
        got = check_case(case)
        for key in ("base", "sub", "ins"):
            assert not np.isnan(got[key]).any(), (case["name"], key)
        if case["name"] == "len 0":
            assert got["base"][1] == 0.0 and got["status"].tolist() == [INFEASIBLE, OK, INFEASIBLE, OK, INFEASIBLE]
            assert got["sub"][0, 0, case["blank"]] == 0.0 and np.isneginf(np.delete(got["sub"][0, 0], case["blank"])).all()
            assert got["ins"][1, 0, case["blank"]] == 0.0 and np.isneginf(got["sub"][2, :2]).all() and np.isneginf(got["ins"][2, :3]).all()


@functools.lru_cache(maxsize=None)
def _identity_batch():
    rs = np.random.default_rng(9)
    T, B, Cn, stride, Lmax, blank = 20, 4, 7, 9, 6, 2
    rows = [[0, 1, 3, 3, 4], [5, 6], [], [1, 0, 1, 0, 1, 6]]
    ids, nids = _pack(rows, stride)
    ids[:, Lmax:] = 99          # never read
    return dict(name="identities", lp=_posteriors(rs, T, B, Cn), lens=[20, 13, 8, 17], ids=ids, nids=nids, Lmax=Lmax, blank=blank,
                entries=None), rows


@pytest.mark.gpu
def test_identities():
    import torch
    from ctc_attention_mispronunciation_amd.hip_model import ctc_loss
    case, rows = _identity_batch()
    got = check_case(case)
    Lmax, blank = case["Lmax"], case["blank"]
    for b, y in enumerate(rows):
        for i, k in enumerate(y):
            assert bits(got["sub"][b, i, k]) == bits(got["base"][b])
        for g in range(len(y) + 1):
            assert bits(got["ins"][b, g, blank]) == bits(got["base"][b])
        assert np.isneginf(got["sub"][b, len(y):Lmax]).all() and np.isneginf(got["ins"][b, len(y) + 1:Lmax + 1]).all()
        assert (got["sub"][b, Lmax:] == SENTINEL).all() and (got["ins"][b, Lmax + 1:] == SENTINEL).all()
    tg = torch.from_numpy(np.where(case["ids"] == 99, 0, case["ids"]).astype(np.int64))
    nll, _ = ctc_loss(torch.from_numpy(case["lp"]).cuda(), tg, torch.tensor(case["lens"]), torch.from_numpy(case["nids"].astype(np.int64)),
                      blank=blank, want_grad=False)
    np.testing.assert_allclose(got["base"], -nll.cpu().numpy().astype(np.float64), rtol=1e-6, atol=0)


@pytest.mark.gpu
def test_bad_and_infeasible_rows_leave_their_neighbours_alone():
    case, rows = _identity_batch()
    Lmax, blank = case["Lmax"], case["blank"]
    clean = gpu_variants(case["lp"], case["lens"], case["ids"], case["nids"], Lmax, blank)

    def same_bits(got, b):
        for key in ("base", "sub", "ins"):
            np.testing.assert_array_equal(bits(got[key][b]), bits(clean[key][b]), err_msg="%s of utterance %d" % (key, b))

    def all_nan(got, b):
        assert np.isnan(got["base"][b]) and np.isnan(got["sub"][b, :Lmax]).all() and np.isnan(got["ins"][b, :Lmax + 1]).all()
        assert (got["sub"][b, Lmax:] == SENTINEL).all() and (got["ins"][b, Lmax + 1:] == SENTINEL).all()

    # a blank among the labels of utterance 0; six equal labels (they need 11 frames) in the 9 frames of utterance 3
    ids, lens = case["ids"].copy(), list(case["lens"])
    ids[0, 2] = blank
    ids[3, :6] = 1; lens[3] = 9
    got = gpu_variants(case["lp"], lens, ids, case["nids"], Lmax, blank)
    assert got["status"].tolist() == [BAD, OK, OK, INFEASIBLE]
    all_nan(got, 0)
    same_bits(got, 1); same_bits(got, 2)
    assert np.isneginf(got["base"][3]) and np.isfinite(got["sub"][3, 2, 0])       # 1 1 0 1 1 1 fits 9 frames: scored on its own
    sl = dict((k, v[1:]) for k, v in got.items())
    worst, _ = compare(sl, case["lp"][:, 1:], lens[1:], ids[1:], case["nids"][1:], blank, None)
    assert worst <= BOUND
    # a label >= C, a count past Lmax and a negative label around utterance 3
    ids, nids = case["ids"].copy(), case["nids"].copy()
    ids[0, 0] = 7; nids[1] = Lmax + 1; ids[2, 0] = -1; nids[2] = 1
    got = gpu_variants(case["lp"], case["lens"], ids, nids, Lmax, blank)
    assert got["status"].tolist() == [BAD, BAD, BAD, OK]
    for b in range(3):
        all_nan(got, b)
    same_bits(got, 3)
    got = gpu_variants(case["lp"], case["lens"], ids, np.array([-1, 2, 0, 6], np.int32), Lmax, blank)
    assert got["status"].tolist() == [BAD, OK, OK, OK]
    same_bits(got, 1); same_bits(got, 2); same_bits(got, 3)


@pytest.mark.gpu
def test_workspace_forms_and_repeat_calls_give_the_same_bits():
    import torch
    case, _ = _identity_batch()
    args = (case["lp"], case["lens"], case["ids"], case["nids"], case["Lmax"], case["blank"])
    first = gpu_variants(*args)
    for other in (gpu_variants(*args), gpu_variants(*args, ws=None), gpu_variants(*args, want_ins=False)):
        for key in ("base", "sub", "status"):
            np.testing.assert_array_equal(bits(other[key]), bits(first[key]), err_msg=key)
    np.testing.assert_array_equal(bits(gpu_variants(*args, ws=None)["ins"]), bits(first["ins"]))
    assert (gpu_variants(*args, want_ins=False)["ins"] == SENTINEL).all()
    L_ = _lib()
    T, B, Cn = case["lp"].shape
    need = L_.mdd_ctc_variants_workspace_bytes(T, B, Cn, case["Lmax"])
    small = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    assert L_.mdd_ctc_variants(p, T, B, Cn, p, p, 9, p, case["Lmax"], case["blank"], p, p, p, p, C.c_void_p(small.data_ptr()), small.numel(), None) == -1
    assert "workspace" in L_.mdd_last_error().decode()
    torch.cuda.synchronize()
    assert not buf.any()        # refused before any device work


@pytest.mark.gpu
def test_chained_from_decode_and_infer_with_posteriors():
    """Greedy ids of a synthetic model's posteriors through ``phoneme_posteriors`` (G13's batch, as tests/test_timed_diagnosis.py), then
    ``infer(..., posteriors=True)``: the flag-less output plus exactly one 'post   :' line per block."""
    import torch
    from tests.test_infer_batch import _case, _read_wav
    from tests.helpers import GOLD, jload
    from ctc_attention_mispronunciation_amd import infer_core, synth
    from ctc_attention_mispronunciation_amd.hip_model import HipModel, ctc_variants
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder, GreedyDecoder, phoneme_posteriors
    from ctc_attention_mispronunciation_amd.utils.data_loader import WavBatchLoader, frames_from_fraction
    meta = jload("g13_infer.json")
    case = _case(meta, 64)
    geom = synth.Geometry(**synth.REFERENCE)
    hip = HipModel(geom, synth.synth_state_dict(geom, seed=11))
    seen = []

    def model(inputs, trans):
        probs = hip.forward(inputs.to("cuda", torch.float32).contiguous(), trans.to("cuda", torch.int64).contiguous(), sync_errors=True)
        seen.append(probs)
        return probs

    i2c = synth.phone_table_41()
    vocab = types.SimpleNamespace(index2word=i2c, word2index={v: k for k, v in i2c.items()})
    beam = BeamDecoder(i2c, beam_width=10, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=0.0)
    phonetic = types.SimpleNamespace(api_word_translation=lambda utterance: "")
    word_dict = {u: {"ipa": meta["utts"][u]["cmu"]} for u in meta["order"]}
    words = {u: meta["utts"][u]["word"] for u in meta["order"]}
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt")))
    loader = WavBatchLoader([(u, _read_wav(int(u)), meta["utts"][u]["canonical"]) for u in meta["order"]], vocab, 64, cmvn)

    def run(**kw):
        buf = io.StringIO()
        totals = infer_core.infer(phonetic, word_dict, loader, torch.device("cuda"), model, beam, vocab, words, False, out=buf, **kw)
        assert list(totals) == case["totals"]
        return buf.getvalue()

    plain = run()
    assert plain == case["stdout"]
    got = run(posteriors=True)
    lines = got.split("\n")
    assert "\n".join(l for l in lines if not l.startswith("post   : ")) == plain
    blocks = got.split("id     : ")[1:]
    assert len(blocks) == len(meta["order"])
    for block in blocks:
        bl = block.split("\n")
        assert bl[11].startswith("score  : ") and bl[12].startswith("post   : ") and bl[13] == ""
        assert sum(l.startswith("post   : ") for l in bl) == 1
        toks = bl[12][9:].split("] ")
        assert [t.split("[")[0] for t in toks] == [p for p in bl[4].split() if p != "I"]
    both = run(posteriors=True, timestamps=True).split("id     : ")[1].split("\n")
    assert both[12].startswith("time   : ") and both[13].startswith("gop    : ") and both[14].startswith("post   : ") and both[15] == ""

    # the greedy decode of the same posteriors, chained with no conversion
    probs = seen[0]
    for inputs, input_sizes, *_ in loader:
        lens = frames_from_fraction(input_sizes, probs.size(0)).numpy().tolist()
        break
    ids, nids = GreedyDecoder(i2c, space_idx=-1, blank_index=0).decode_ids(probs, lens)
    post = phoneme_posteriors(probs, lens, ids, nids, 0)
    r = ctc_variants(probs, torch.tensor(lens), ids, nids, blank=0, max_len=int(nids.max()))
    n, ids_h, sub, ins = nids.cpu().numpy(), ids.cpu().numpy(), r.sub.cpu().numpy(), r.ins.cpu().numpy()
    assert (r.status.cpu().numpy() == OK).all() and all(p is not None for p in post)
    checked = 0
    for b in range(len(lens)):
        positions, gaps = post[b]
        assert len(positions) == n[b] and len(gaps) == n[b] + 1
        for i, (p_ok, p_del, alt, p_alt) in enumerate(positions):
            row = sub[b, i]
            e = np.exp(row - row.max())
            sm = e / e.sum()
            assert abs(sm.sum() - 1.0) <= 1e-12 and abs(p_ok + p_del + np.delete(sm, [0, ids_h[b, i]]).sum() - 1.0) <= 1e-12
            assert abs(p_ok - sm[ids_h[b, i]]) <= 1e-12 and abs(p_del - sm[0]) <= 1e-12 and abs(p_alt - sm[alt]) <= 1e-12
            assert alt not in (0, ids_h[b, i]) and p_alt == max(sm[k] for k in range(len(sm)) if k not in (0, ids_h[b, i]))
            checked += 1
        for g, (k_ins, p_ins) in enumerate(gaps):
            row = ins[b, g]
            e = np.exp(row - row.max())
            sm = e / e.sum()
            assert abs(sm.sum() - 1.0) <= 1e-12 and k_ins != 0 and p_ins == sm[k_ins] and p_ins == np.delete(sm, 0).max()
            assert abs(sm[0] + p_ins + np.delete(sm, [0, k_ins]).sum() - 1.0) <= 1e-12      # "nothing inserted" + every insertion
    assert checked > 0
