"""Float64 references for the best reading of an error network (mdd_ctc_confnet_best, DESIGN.md "Best reading").

``brute_best``  every reading enumerated, each through a Viterbi CTC alignment of the labels it emits.
``best_f64``    the max-product state recurrences of DESIGN.md with backpointers and a backtrace, float64 numpy, the chain along the slots
                walked slot by slot (no block fold): score, reading, seg and path.
``rescore``     what a returned (reading, seg) is worth, or None when it is no reading of the network with a CTC path."""
import itertools

import numpy as np

NEG = -np.inf


def viterbi(lp, Tb, labels, blank):
    """The best CTC path's log-probability of ``labels`` over the first Tb frames of lp [T, C], float64; -inf without a path."""
    lp = np.asarray(lp, dtype=np.float64)[:Tb]
    L = len(labels)
    if Tb == 0:
        return 0.0 if L == 0 else NEG
    ext = [blank] * (2 * L + 1)
    ext[1::2] = labels
    a = np.full(2 * L + 1, NEG)
    a[0] = lp[0, blank]
    if L:
        a[1] = lp[0, ext[1]]
    for t in range(1, Tb):
        n = np.full(2 * L + 1, NEG)
        for s in range(2 * L + 1):
            v = a[s]
            if s >= 1:
                v = max(v, a[s - 1])
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                v = max(v, a[s - 2])
            n[s] = v + lp[t, ext[s]]
        a = n
    return float(max(a[-1], a[-2]) if L else a[-1])


def brute_best(lp, Tb, w, blank):
    """(score, reading) by enumeration: the largest sum of a reading's weights and the Viterbi score of its labels; (-inf, None) when no
    reading has a path.  lp [T, C], the first Tb frames count; w [J, C] log-weights, -inf = no arc."""
    w = np.asarray(w, dtype=np.float64)
    J, C = w.shape
    arcs = [[k for k in range(C) if w[j, k] > NEG] for j in range(J)]
    memo = {}
    best, arg = NEG, None
    for r in itertools.product(*arcs):          # J = 0: the one empty reading
        labels = tuple(k for k in r if k != blank)
        if labels not in memo:
            memo[labels] = viterbi(lp, Tb, list(labels), blank)
        s = sum(w[j, k] for j, k in enumerate(r)) + memo[labels]
        if s > best:
            best, arg = s, list(r)
    return float(best), arg


def best_f64(lp, Tb, w, blank):
    """(score, reading [J], seg [J, 2], path [Tb]) by the recurrences of DESIGN.md "Best reading"; (-inf, None, None, None) when no reading
    has a path.  Ties: staying over entering, the nearer slot over skipping, the lower class."""
    w = np.asarray(w, dtype=np.float64)
    J, C = w.shape
    lp = np.asarray(lp, dtype=np.float64)[:Tb]
    T = len(lp)
    rows = np.arange(J)
    skip = w[:, blank]
    pre = np.concatenate([[0.0], np.cumsum(skip)])
    X = np.full((J, C), NEG)
    E = np.repeat(pre[:J, None], C, axis=1)
    enter = np.zeros((T, J, C), dtype=bool)
    source = np.zeros((T, J, C), dtype=bool)
    top = np.zeros((T, J, 2), dtype=np.int64)
    blk = 0.0
    for t in range(T):
        allp = X.max(axis=1) if J else np.zeros(0)
        en = w + E
        enter[t] = en > X
        Xn = lp[t][None, :] + np.where(enter[t], en, X)
        Xn[:, blank] = lp[t, blank] + allp
        X = Xn
        i1 = X.argmax(axis=1) if J else np.zeros(0, dtype=np.int64)
        m1 = X[rows, i1]
        rest = X.copy()
        rest[rows, i1] = NEG
        i2 = rest.argmax(axis=1) if J else i1
        i2 = np.where(i2 == i1, (i1 + 1) % C, i2)           # everything else at -inf: any other class, never followed
        m2 = rest[rows, i2]
        top[t, :, 0], top[t, :, 1] = i1, i2
        src = np.where(np.arange(C)[None, :] == i1[:, None], m2[:, None], m1[:, None])
        blk += lp[t, blank]
        e = np.full(C, blk)
        for j in range(J):
            E[j] = e
            source[t, j] = src[j] >= skip[j] + e
            e = np.where(source[t, j], src[j], skip[j] + e)
    last = X.max(axis=1) if J and T else np.full(J, NEG)
    end = np.empty(J + 1)
    end[0] = blk
    for j in range(J):
        end[j + 1] = max(skip[j] + end[j], last[j])
    if not end[J] > NEG:
        return NEG, None, None, None
    reading = [blank] * J
    seg = [[-1, -1] for _ in range(J)]
    path = [-1] * T
    j, t, k, state = J, T - 1, blank, False
    while j > 0 and not state:
        j -= 1
        if last[j] >= skip[j] + end[j]:
            state, k = True, int(top[t, j, 0])
    seg_end = -1
    while state:
        if k == blank:
            k = int(top[t - 1, j, 0])
            t -= 1
            continue
        path[t] = j
        if seg_end < 0:
            seg_end, reading[j] = t + 1, k
        entered = bool(enter[t, j, k])
        t -= 1
        if not entered:
            continue
        seg[j] = [t + 1, seg_end]
        seg_end, state = -1, False
        if t < 0:
            break
        while j > 0:
            j -= 1
            if source[t, j, k]:
                i1, i2 = int(top[t, j, 0]), int(top[t, j, 1])
                k = i1 if i1 != k else i2
                state = True
                break
    return float(end[J]), reading, seg, path


def rescore(lp, Tb, w, blank, reading, seg):
    """The reading's weights, plus lp of its labels over their segments, plus lp[., blank] on every other frame below Tb (float64).  None
    unless the reading uses existing arcs, the segments are ordered, disjoint and inside [0, Tb), equal neighbouring labels have a blank
    frame between them, and slots that emit nothing have (-1, -1)."""
    w = np.asarray(w, dtype=np.float64)
    lp = np.asarray(lp, dtype=np.float64)
    J, C = w.shape
    if len(reading) != J or len(seg) != J:
        return None
    total = 0.0
    used = np.zeros(Tb, dtype=bool)
    prev_end, prev_label = 0, None
    for j in range(J):
        k, (s, e) = int(reading[j]), (int(seg[j][0]), int(seg[j][1]))
        if not 0 <= k < C or not w[j, k] > NEG:
            return None
        total += w[j, k]
        if k == blank:
            if (s, e) != (-1, -1):
                return None
            continue
        if not (prev_end <= s < e <= Tb):
            return None
        if prev_label == k and s == prev_end:
            return None
        total += lp[s:e, k].sum()
        used[s:e] = True
        prev_end, prev_label = e, k
    total += lp[:Tb, blank][~used].sum()
    return float(total)


def path_of(seg, J, Tb, T):
    """The path [T] a seg [J, 2] stands for: the slot per frame, -1 on blank frames and from Tb on."""
    path = np.full(T, -1, dtype=np.int64)
    for j in range(J):
        if seg[j][0] >= 0:
            path[seg[j][0]:seg[j][1]] = j
    return path
