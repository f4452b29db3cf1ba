"""Float64 references for CTC over an error network (mdd_ctc_confnet, DESIGN.md "Error network").

``brute``          every reading enumerated; the labels it emits go through CPU ``ctc_loss`` in double (tests/test_ctc_variants.py::brute).
``lattice_f64``    the state recurrence of DESIGN.md written label / blank apart, log domain, float64 numpy, forward only: total of a network (or of a
                   batch of networks over the same posteriors).
``marginals_f64``  post[j, k] as the total of the network whose row j is cut down to entry k -- no backward sweep, so it shares nothing
                   with the kernel's way of getting the marginals.
Log-sums "over all but k" are prefix / suffix accumulations; nothing is subtracted, so an absent reading is exactly -inf."""
import itertools

import numpy as np

NEG = -np.inf


def brute(lp, Tb, w, blank):
    """(total, post [J, C]) by enumeration.  lp [T, C], the first Tb frames count; w [J, C] log-weights, -inf = no arc."""
    from tests.test_ctc_variants import brute as ctc_brute
    w = np.asarray(w, dtype=np.float64)
    J, C = w.shape
    arcs = [[k for k in range(C) if w[j, k] > NEG] for j in range(J)]
    readings = list(itertools.product(*arcs))           # J = 0: the one empty reading
    post = np.full((J, C), NEG)
    if not readings:
        return NEG, post
    strings = sorted({tuple(k for k in r if k != blank) for r in readings})
    ll = dict(zip(strings, ctc_brute(lp, Tb, [list(s) for s in strings], blank)))
    score = np.array([sum(w[j, k] for j, k in enumerate(r)) + ll[tuple(k for k in r if k != blank)] for r in readings])
    pick = np.array(readings, dtype=np.int64).reshape(len(readings), J)
    for j in range(J):
        for k in arcs[j]:
            post[j, k] = np.logaddexp.reduce(score[pick[:, j] == k])
    return float(np.logaddexp.reduce(score)), post


def _excl(a):
    """log-sum over the last axis of every entry but the own one: prefix (+) suffix, no subtraction."""
    out = np.full(a.shape, NEG)
    if a.shape[-1] > 1:
        out[..., 1:] = np.logaddexp.accumulate(a, axis=-1)[..., :-1]
        suf = np.logaddexp.accumulate(a[..., ::-1], axis=-1)[..., ::-1]
        out[..., :-1] = np.logaddexp(out[..., :-1], suf[..., 1:])
    return out


def lattice_f64(lp, Tb, w, blank):
    """total of the network w [J, C] -- or of each of the N networks w [N, J, C] -- over the first Tb frames of lp [T, C]."""
    w = np.asarray(w, dtype=np.float64)
    single = w.ndim == 2
    if single:
        w = w[None]
    N, J, C = w.shape
    lp = np.asarray(lp, dtype=np.float64)[:Tb]
    lab = np.arange(C) != blank
    W = np.where(lab, w, NEG)                # label arcs; the blank entry is the skip
    skip = w[:, :, blank]                    # [N, J]
    Lab = np.full((N, J, C), NEG)            # Lab_t(j, k)
    Blk = np.full((N, J), NEG)               # Blk_t(j)
    Blk0 = np.zeros(N)                       # Blk_t(-1); 1 before frame 0

    def entry():
        """E_t(j, k) from the states of frame t: the only recurrence along the slots."""
        src = np.logaddexp(Blk[:, :, None], _excl(Lab))
        E = np.empty((N, J, C))
        e = np.repeat(Blk0[:, None], C, axis=1)
        for j in range(J):
            E[:, j] = e
            e = np.logaddexp(skip[:, j, None] + e, src[:, j])
        return E

    for t in range(len(lp)):
        E = entry()
        allj = np.logaddexp(Blk, np.logaddexp.reduce(Lab, axis=2)) if C else Blk
        Lab = np.where(lab, lp[t][None, None, :] + np.logaddexp(Lab, W + E), NEG)
        Blk = lp[t, blank] + allj
        Blk0 = Blk0 + lp[t, blank]
    tail = np.zeros((N, J + 1))              # tail[:, j + 1] = sum_{m > j} skip_m
    for j in range(J - 1, -1, -1):
        tail[:, j] = tail[:, j + 1] + skip[:, j]
    ends = np.concatenate([Blk0[:, None], np.logaddexp(Blk, np.logaddexp.reduce(Lab, axis=2))], axis=1)
    total = np.logaddexp.reduce(tail + ends, axis=1)
    return float(total[0]) if single else total


def marginals_f64(lp, Tb, w, blank, entries=None):
    """post of the listed (j, k) entries (default: all, as a [J, C] array; a list gives a vector): the total of the network whose row j
    is cut down to entry k."""
    w = np.asarray(w, dtype=np.float64)
    J, C = w.shape
    ent = [(j, k) for j in range(J) for k in range(C)] if entries is None else list(entries)
    out = np.full(len(ent), NEG)
    step = max(1, 2000000 // max(J * C, 1))
    for n0 in range(0, len(ent), step):
        part = ent[n0:n0 + step]
        cut = np.repeat(w[None], len(part), axis=0)
        for n, (j, k) in enumerate(part):
            keep = cut[n, j, k]
            cut[n, j, :] = NEG
            cut[n, j, k] = keep
        out[n0:n0 + step] = lattice_f64(lp, Tb, cut, blank)
    return out.reshape(J, C) if entries is None else out


def forward_backward_f64(lp, Tb, w, blank):
    """(total, post [J, C]) by the forward / backward sweeps of DESIGN.md "Error network" -- the kernel's scheme in float64, so that a GPU
    failure can be told apart from a wrong formula.  X[j, blank] is the blank state after slot j's label."""
    w = np.asarray(w, dtype=np.float64)
    J, C = w.shape
    lp = np.asarray(lp, dtype=np.float64)[:Tb]
    T = len(lp)
    lab = np.arange(C) != blank
    lae = np.logaddexp
    skip = w[:, blank]
    pre = np.concatenate([[0.0], np.cumsum(skip)])                     # pre[j] = sum_{m < j} skip_m
    tail = np.concatenate([np.cumsum(skip[::-1])[::-1], [0.0]])[1:] if J else np.zeros(0)     # tail[j] = sum_{m > j} skip_m

    def chain(first, src):
        E = np.empty((J, C))
        e = np.full(C, first)
        for j in range(J):
            E[j] = e
            e = lae(skip[j] + e, src[j])
        return E, e

    X = np.full((J, C), NEG)
    E = np.repeat(pre[:J, None], C, axis=1)
    Es, blk = [E], 0.0                                                   # Es[t] = E_{t-1}
    for t in range(T):
        allj = lae.reduce(X, axis=1)
        X = np.where(lab, lp[t][None, :] + lae(X, w + E), (lp[t, blank] + allj)[:, None])
        blk += lp[t, blank]
        E, _ = chain(blk, _excl(X))
        Es.append(E)
    end, total = chain(blk, np.repeat(lae.reduce(X, axis=1)[:, None], C, axis=1))
    end, total = end[:, 0], float(total[0])
    post = np.full((J, C), NEG)
    if J:
        post[:, blank] = end + skip + tail
    Y = lp[T - 1][None, :] + tail[:, None] if T else None
    for t in range(T - 1, -1, -1):                                       # the transition into frame t
        F = np.full((J + 1, C), NEG)
        for j in range(J - 1, -1, -1):
            F[j] = np.where(lab, lae(w[j] + Y[j], skip[j] + F[j + 1]), NEG)
        Fn = F[1:]
        post = np.where(lab, lae(post, w + Es[t] + Y), post)
        over = lae.reduce(np.where(lab, Es[t] + skip[:, None] + Fn, NEG), axis=1)
        post[:, blank] = lae(post[:, blank], over)
        if t > 0:
            V = np.where(lab, Fn, Y[:, blank][:, None])
            Y = np.where(lab, lp[t - 1][None, :] + lae(Y, _excl(V)), (lp[t - 1, blank] + lae.reduce(V, axis=1))[:, None])
    return total, post


# ------------------------------------------------------------------------------------------------------------ shared inputs
def posteriors(rs, T, Cn, scale=2.0):
    """[T, C] float32 log-softmax rows."""
    x = rs.standard_normal((T, Cn)) * scale
    x = x - np.log(np.exp(x).sum(axis=-1, keepdims=True))
    return x.astype(np.float32)


def random_network(rs, J, Cn, absent=0.3, scale=1.5):
    """[J, C] float32 log-weights, a share ``absent`` of the arcs at -inf (a whole row may go)."""
    w = (rs.standard_normal((J, Cn)) * scale).astype(np.float32)
    w[rs.random((J, Cn)) < absent] = NEG
    return w


def canonical_network(y, Cn, blank, open_slots=()):
    """The 2L+1 slots of the canonical y: gaps "blank only, 0", positions "own label only, 0"; the slots listed in open_slots get all C
    entries at weight 0."""
    L = len(y)
    w = np.full((2 * L + 1, Cn), NEG, dtype=np.float32)
    w[0::2, blank] = 0.0
    for i, k in enumerate(y):
        w[2 * i + 1, k] = 0.0
    for j in open_slots:
        w[j, :] = 0.0
    return w
