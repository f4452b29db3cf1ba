"""The yardstick of mdd_nbest_mbr -- TEST INFRASTRUCTURE, CPU only.

``distance`` is the definition: the unit-cost Levenshtein distance by the two-row DP in pure Python, an empty side giving the other
side's length.  ``reference`` restates the entry's contract (include/mdd_hip.h) on host arrays: the flag rules, ``dist``, ``risk`` by
``math.fsum``, the ``best`` rule (the lowest rank with a weight above 0 and the least risk), ``ref_dist`` / ``ref_risk``.  It also
returns, per risk entry, sum_m w_m d(n, m): what the bound of a differently ordered fp64 sum is made of.

``pair_distances`` is the same DP for all pairs of two padded lists at once in numpy (one row of the matrix per step, the in-row
dependency D[i][j-1] + 1 resolved as j + cummin(tmp[k] - k)); ``reference`` uses it so that N = 256 stays quick, and
tests/test_mbr_reference.py holds it to ``distance`` pair by pair.

The module also draws the inputs: N-best-like lists (a random base sequence with a few random edits per hypothesis, some rows
duplicated), rows of exact lengths, the weights, and the poison behind every row's length.
"""
import math

import numpy as np

MAX_N, MAX_LEN = 256, 1024
POISON = (2 ** 30, -1)


def distance(a, b):
    """Unit-cost Levenshtein distance of two sequences: two rows of the DP matrix."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y))
        prev = cur
    return prev[len(b)]


def pair_distances(P, plen, T, tlen):
    """d(P[x, :plen[x]], T[y, :tlen[y]]) for every x, y as an int32 [len(plen), len(tlen)] array.  Cells past a row's length are
    computed from the padding and never read: D[i][j] depends on the two prefixes alone."""
    P, T = np.asarray(P, dtype=np.int32), np.asarray(T, dtype=np.int32)
    plen, tlen = np.asarray(plen, dtype=np.int64), np.asarray(tlen, dtype=np.int64)
    n, m = len(plen), len(tlen)
    Lt = int(tlen.max()) if m else 0
    T = T[:, :Lt]
    j = np.arange(Lt + 1, dtype=np.int32)
    cols = np.arange(m)
    prev = np.broadcast_to(j, (n, m, Lt + 1)).copy()
    out = np.zeros((n, m), dtype=np.int32)
    out[plen == 0] = tlen
    for i in range(1, (int(plen.max()) if n else 0) + 1):
        tmp = np.empty_like(prev)
        tmp[..., 0] = i
        cost = P[:, i - 1][:, None, None] != T[None, :, :]
        tmp[..., 1:] = np.minimum(prev[..., 1:] + 1, prev[..., :-1] + cost)
        prev = np.minimum.accumulate(tmp - j, axis=-1) + j
        rows = np.nonzero(plen == i)[0]
        if len(rows):
            out[rows] = prev[rows][:, cols, tlen]
    return out


def reference(ids, nids, status, weights, C, max_len, ref=None, ref_len=None):
    """The contract of mdd_nbest_mbr on host arrays: ids [N,B,pitch], nids [N,B], status [B] or None, weights [N,B] float64, ref
    [B,ref_pitch] / ref_len [B] or None.  Returns a dict of best [B], risk [N,B], flag [B], dist [B,N,N], ref_dist [N,B], ref_risk [B]
    (the last two None without a reference) and mass [N,B] / ref_mass [B] = the sums of the non-negative terms w_m d behind each risk."""
    ids, nids, weights = np.asarray(ids), np.asarray(nids), np.asarray(weights, dtype=np.float64)
    N, B, pitch = ids.shape
    assert 1 <= N <= MAX_N and 1 <= max_len <= min(pitch, MAX_LEN) and 2 <= C <= 256
    has_ref = ref is not None
    out = dict(best=np.full(B, -1, np.int32), risk=np.full((N, B), np.nan), flag=np.zeros(B, np.int32), dist=np.full((B, N, N), -1, np.int32),
               ref_dist=np.full((N, B), -1, np.int32) if has_ref else None, ref_risk=np.full(B, np.nan) if has_ref else None,
               mass=np.zeros((N, B)), ref_mass=np.zeros(B))
    for b in range(B):
        if status is not None and status[b] != 0:
            out["flag"][b] = 1
            continue
        rows = [(ids[n, b], int(nids[n, b]), max_len) for n in range(N)]
        if has_ref:
            rows.append((np.asarray(ref)[b], int(ref_len[b]), min(max_len, np.asarray(ref).shape[1])))
        if any(not 0 <= ln <= cap or any(not 0 <= int(v) < C for v in row[:ln]) for row, ln, cap in rows):
            out["flag"][b] = 2
            continue
        w = weights[:, b]
        if not (w > 0).any():
            out["flag"][b] = 1
            continue
        lens = np.array([ln for _, ln, _ in rows])
        width = max(int(lens.max()), 1)
        pad = np.zeros((len(rows), width), dtype=np.int64)
        for x, (row, ln, _) in enumerate(rows):
            pad[x, :ln] = row[:ln]
        d = pair_distances(pad, lens, pad[:N], lens[:N])
        out["dist"][b] = d[:N]
        for n in range(N):
            terms = [float(w[m]) * float(d[n, m]) for m in range(N)]
            out["risk"][n, b] = math.fsum(terms)
            out["mass"][n, b] = math.fsum(terms)
        cand = [n for n in range(N) if w[n] > 0]
        out["best"][b] = min(cand, key=lambda n: (out["risk"][n, b], n))
        if has_ref:
            out["ref_dist"][:, b] = d[N]
            terms = [float(w[m]) * float(d[N, m]) for m in range(N)]
            out["ref_risk"][b] = out["ref_mass"][b] = math.fsum(terms)
    return out


# ------------------------------------------------------------------------------------------------------------------ inputs
def edited(rs, base, C, max_len, edits):
    seq = list(base)
    for _ in range(edits):
        op, at = rs.integers(0, 3), int(rs.integers(0, len(seq) + 1))
        if op == 0 and at < len(seq):
            seq[at] = int(rs.integers(0, C))
        elif op == 1:
            seq.insert(at, int(rs.integers(0, C)))
        elif at < len(seq):
            del seq[at]
    return seq[:max_len]


def draw_lists(seed, N, B, C, max_len, pitch=None, exact=(), top_id=False):
    """(ids [N,B,pitch] int32, nids [N,B] int32): per utterance a random base sequence and, per hypothesis, 0-3 random edits of it;
    about one row in seven repeats an earlier row of its utterance.  ``exact``: lengths that rows (n, b) = (x % N, x % B) for x = 0, 1, ..
    take exactly, with random ids (so that rows of exactly max_len, 0 and 1 ids sit next to the others).  ``top_id``: id C - 1 is put
    into row 0 of every utterance that has an id at all.  Behind a row's length the ids are 0."""
    rs = np.random.default_rng(seed)
    pitch = max_len + 3 if pitch is None else pitch
    ids, nids = np.zeros((N, B, pitch), dtype=np.int32), np.zeros((N, B), dtype=np.int32)
    for b in range(B):
        base = rs.integers(0, C, size=int(rs.integers(max(1, max_len // 2), max_len + 1))).tolist()
        for n in range(N):
            seq = edited(rs, base, C, max_len, int(rs.integers(0, 4)))
            if n and rs.random() < 0.15:
                k = int(rs.integers(0, n))
                seq = ids[k, b, :nids[k, b]].tolist()
            ids[n, b, :len(seq)], nids[n, b] = seq, len(seq)
    for x, ln in enumerate(exact):
        n, b = x % N, x % B
        ids[n, b] = 0
        ids[n, b, :ln], nids[n, b] = rs.integers(0, C, size=ln), ln
    if top_id:
        for b in range(B):
            if nids[0, b]:
                ids[0, b, int(rs.integers(0, nids[0, b]))] = C - 1
    return ids, nids


def poisoned(seed, ids, nids, C):
    """A copy of ids with everything behind each row's length replaced: 2^30, -1 and valid ids, at random."""
    rs = np.random.default_rng(seed)
    out = ids.copy()
    fill = rs.choice(np.array(POISON + (0, C - 1, 1), dtype=np.int64), size=ids.shape).astype(np.int32)
    tail = np.arange(ids.shape[2])[None, None, :] >= nids[:, :, None]
    out[tail] = fill[tail]
    return out


def exact_weights(seed, N, B):
    """Weights k / 2^10 with small k (some 0): every product with a distance below 2^11 and every sum of N <= 256 of them is exact in
    fp64, whatever the order."""
    rs = np.random.default_rng(seed)
    w = rs.integers(0, 9, size=(N, B)).astype(np.float64) / 1024.0
    w[0, w.sum(axis=0) == 0] = 1.0 / 1024.0
    return w


def softmax_weights(seed, N, B, dead=0.2):
    """What nbest_posteriors gives: the float64 softmax of random log-likelihoods per utterance, about ``dead`` of them -inf (weight 0),
    at least one alive."""
    rs = np.random.default_rng(seed)
    ll = -rs.uniform(5.0, 40.0, size=(N, B))
    ll[rs.random((N, B)) < dead] = -np.inf
    for b in range(B):
        if not np.isfinite(ll[:, b]).any():
            ll[int(rs.integers(0, N)), b] = -7.0
    with np.errstate(under="ignore"):
        e = np.exp(ll - ll.max(axis=0))
    return e / e.sum(axis=0)
