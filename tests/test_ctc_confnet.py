"""CTC over an error network on the GPU (mdd_ctc_confnet, csrc/ctc_confnet.hip) against the float64 references of
tests/confnet_reference.py: the enumeration of all readings (``brute``) on tiny networks, and ``lattice_f64`` / ``marginals_f64`` -- checked
against the enumeration on the CPU by tests/test_ctc_confnet_reference.py -- at the smallest shapes where the kernel's structure changes.

Numeric bound (finite entries, absolute): BOUND = 4 x the largest error measured over ``all_cases()`` on an MI355X by
tools/ctc_confnet_margins.py (profiles/ctc_confnet_margins.json: 6.6e-7 over 3,247 finite entries), the factor 4 for input-dependent rounding, and never past the project's
1e-4 log-prob tolerance -- the scheme of tests/test_ctc_variants.py.  -inf positions must be the reference's exactly.  Against
mdd_ctc_variants the bound is this BOUND plus that module's own; for logsumexp_k post[j, :] == total it is 2 BOUND, both sides being
within BOUND of the same exact number."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import confnet_reference as ref

NEG = -np.inf
OK, INFEASIBLE, BAD = 0, 1, 2
SENTINEL = 12345.0
CAP = 1e-4
MEASURED_MAX = 6.65e-7      # profiles/ctc_confnet_margins.json "confnet_max_abs_err", rounded up
BOUND = min(4 * MEASURED_MAX, CAP)


def _lib():
    from ctc_attention_mispronunciation_amd import _lib
    return _lib.lib()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------------------ the device call
def gpu_confnet(lp, lens, w, nslots, Jmax, blank, ws="torch", want_post=True):
    """mdd_ctc_confnet through ctypes on sentinel-filled buffers.  ws: 'torch' (caller workspace of the stated size) or None (NULL)."""
    import torch
    L_ = _lib()
    T, B, Cn = lp.shape
    stride = w.shape[1]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    lp_d, len_d, ns_d = d(lp.astype(np.float32)), d(np.asarray(lens, np.int32)), d(np.asarray(nslots, np.int32))
    w_d = d(w.astype(np.float32)) if stride else torch.zeros(1, dtype=torch.float32, device="cuda")
    total = torch.full((B,), SENTINEL, dtype=torch.float64, device="cuda")
    post = torch.full((B, max(stride, 1), Cn), SENTINEL, dtype=torch.float64, device="cuda")
    status = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    need = L_.mdd_ctc_confnet_workspace_bytes(T, B, Cn, Jmax, 1 if want_post else 0)
    wsbuf = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda") if ws == "torch" else None
    rc = L_.mdd_ctc_confnet(p(lp_d), T, B, Cn, p(len_d), p(w_d), stride, p(ns_d), Jmax, blank, p(total), p(post) if want_post else None,
                            p(status), p(wsbuf) if wsbuf is not None else None, need if wsbuf is not None else 0, None)
    assert rc == 0, L_.mdd_last_error().decode()
    torch.cuda.synchronize()
    return dict(total=total.cpu().numpy(), post=post.cpu().numpy()[:, :stride], status=status.cpu().numpy())


def reference(case, b):
    """(total, entries, post values) of utterance b in float64: by enumeration, or by the lattice on all / the listed entries."""
    lp, w, blank = case["lp"][:, b, :], case["w"][b, :int(case["nslots"][b])], case["blank"]
    T = lp.shape[0]
    Tb = min(max(int(case["lens"][b]), 0), T)
    J, Cn = w.shape
    if case["ref"] == "brute":
        total, post = ref.brute(lp, Tb, w, blank)
        return total, [(j, k) for j in range(J) for k in range(Cn)], post.reshape(-1)
    ent = case["entries"][b] if case.get("entries") else [(j, k) for j in range(J) for k in range(Cn)]
    return ref.lattice_f64(lp, Tb, w, blank), ent, ref.marginals_f64(lp, Tb, w, blank, ent)


def compare(got, case):
    """total, status and every listed post entry of every utterance against the reference: -inf where and only where the reference is,
    finite entries returned as (max |error|, count); rows from nslots to Jmax -inf, rows behind Jmax untouched."""
    worst, count = 0.0, 0
    B = case["lp"].shape[1]
    for b in range(B):
        J = int(case["nslots"][b])
        total, ent, want = reference(case, b)
        have = np.array([got["total"][b]] + [got["post"][b, j, k] for j, k in ent])
        want = np.concatenate([[total], want])
        assert got["status"][b] == (INFEASIBLE if np.isneginf(total) else OK), (case["name"], b, got["status"][b], total)
        wrong = np.isneginf(have) != np.isneginf(want)
        assert not wrong.any(), (case["name"], b, [([("total",)] + ent)[n] for n in np.nonzero(wrong)[0][:5]], have[wrong][:5], want[wrong][:5])
        fin = np.isfinite(want)
        assert np.isfinite(have[fin]).all(), (case["name"], b)
        err = np.abs(have[fin] - want[fin])
        print("%s, utterance %d: J %d, len %d, %d finite entries, max |error| %.3e" % (case["name"], b, J, int(case["lens"][b]), int(fin.sum()),
                                                                                     err.max(initial=0.0)))
        worst, count = max(worst, float(err.max(initial=0.0))), count + int(fin.sum())
        assert np.isneginf(got["post"][b, J:case["Jmax"]]).all() and (got["post"][b, case["Jmax"]:] == SENTINEL).all(), (case["name"], b)
    return worst, count


def run_case(case):
    got = gpu_confnet(case["lp"], case["lens"], case["w"], case["nslots"], case["Jmax"], case["blank"])
    worst, count = compare(got, case)
    return got, worst, count


def check_case(case):
    got, worst, _ = run_case(case)
    assert worst <= BOUND, (case["name"], worst, BOUND)
    return got


# ------------------------------------------------------------------------------------------------------------ the cases
def _batch(rs, T, Cn, nets, stride):
    """lp [T, B, C] and the networks packed into w [B, stride, C]; the rows behind a network hold NaN: they are never read."""
    B = len(nets)
    lp = np.stack([ref.posteriors(rs, T, Cn) for _ in range(B)], axis=1)
    w = np.full((B, stride, Cn), np.nan, dtype=np.float32)
    for b, net in enumerate(nets):
        w[b, :len(net)] = net
    return lp, w, np.array([len(n) for n in nets], np.int32)


def tiny_cases(Cn):
    """The enumerated networks: C classes, every blank index, T = 6, six networks per batch with J in 0..5 and len in 0..6 (a J = 0 and a
    len = 0 among them), two arcs in ten absent."""
    for blank in range(Cn):
        rs = np.random.default_rng(10 * Cn + blank)
        Js = [0, 5, 3] + [int(v) for v in rs.integers(1, 6, size=3)]
        lens = [6, 0, 4] + [int(v) for v in rs.integers(2, 7, size=3)]
        lp, w, nslots = _batch(rs, 6, Cn, [ref.random_network(rs, J, Cn, 0.2) for J in Js], 7)
        yield dict(name="tiny C %d blank %d" % (Cn, blank), lp=lp, lens=lens, w=w, nslots=nslots, Jmax=5, blank=blank, ref="brute")


def _net(rs, J, Cn, blank, absent=0.3):
    """A random network whose skips all exist, so that a short utterance has a path through a long network."""
    w = ref.random_network(rs, J, Cn, absent)
    w[:, blank] = (rs.standard_normal(J) * 1.5).astype(np.float32)
    return w


def _sample(rs, J, Cn, blank, n):
    """Every 'emits nothing' entry and n entries drawn at random."""
    return [(j, blank) for j in range(J)] + [(int(rs.integers(J)), int(rs.integers(Cn))) for _ in range(n)]


def shape_case(name):
    """The smallest shapes at which the kernel takes another path (the marginals of every entry unless sampled)."""
    rs = np.random.default_rng(sum(ord(c) for c in name))
    entries = None
    if name == "C 45":                  # one lane pass; a second utterance with fewer slots and len < T
        T, Cn, blank, Js, lens = 25, 45, 0, [11, 7], [25, 19]
    elif name == "C 45 blank 44":
        T, Cn, blank, Js, lens = 12, 45, 44, [5], [12]
    elif name == "C 65 blank 64":       # the second lane pass holds the blank alone
        T, Cn, blank, Js, lens = 8, 65, 64, [5, 2], [8, 6]
    elif name == "C 65 blank 3":
        T, Cn, blank, Js, lens = 8, 65, 3, [4], [7]
    elif name == "C 130 blank 70":      # three lane passes
        T, Cn, blank, Js, lens = 5, 130, 70, [3], [5]
    elif name == "C 256":               # four full lane passes
        T, Cn, blank, Js, lens = 4, 256, 200, [3, 1], [4, 3]
    elif name == "J 17":                # one slot per wave and one more
        T, Cn, blank, Js, lens = 10, 5, 2, [17, 16], [10, 9]
    elif name == "J max":               # max_slots(45) slots, three frames
        Cn = 45
        J = int(_lib().mdd_ctc_confnet_max_slots(Cn))
        T, blank, Js, lens = 3, 0, [J, J - 1], [3, 2]
        entries = [_sample(rs, n, Cn, blank, 150) for n in Js]
    else:
        raise KeyError(name)
    lp, w, nslots = _batch(rs, T, Cn, [_net(rs, J, Cn, blank) for J in Js], max(Js) + 1)
    return dict(name=name, lp=lp, lens=lens, w=w, nslots=nslots, Jmax=max(Js), blank=blank, ref="lattice", entries=entries)


SHAPES = ("C 45", "C 45 blank 44", "C 65 blank 64", "C 65 blank 3", "C 130 blank 70", "C 256", "J 17", "J max")


def edge_cases():
    rs = np.random.default_rng(5)
    Cn, blank = 4, 1
    # frames >= len are never read: NaN there must not reach any output
    lp, w, nslots = _batch(rs, 7, Cn, [_net(rs, J, Cn, blank) for J in (3, 4, 2)], 5)
    lens = [4, 7, 0]
    for b, n in enumerate(lens):
        lp[n:, b, :] = np.nan
    yield dict(name="NaN past len", lp=lp, lens=lens, w=w, nslots=nslots, Jmax=4, blank=blank, ref="brute")
    # classes the model rules out in every frame, the blank in one utterance; a slot whose only arc is such a class: no reading has a path
    lp, w, nslots = _batch(rs, 6, Cn, [_net(rs, J, Cn, blank) for J in (3, 3, 2)], 4)
    lp[:, 0, 2] = NEG
    lp[:, 1, blank] = NEG
    w[2, 1] = NEG
    w[2, 1, 3] = 0.0
    lp[:, 2, 3] = NEG
    yield dict(name="classes at -inf", lp=lp, lens=[6, 6, 5], w=w, nslots=nslots, Jmax=3, blank=blank, ref="brute")
    # T = 1 and len = 1
    lp, w, nslots = _batch(rs, 1, Cn, [_net(rs, J, Cn, blank) for J in (1, 3, 0)], 3)
    yield dict(name="T 1", lp=lp, lens=[1, 1, 1], w=w, nslots=nslots, Jmax=3, blank=blank, ref="brute")


def all_cases():
    """Every case the bound is measured over (tools/ctc_confnet_margins.py)."""
    for Cn in (2, 3, 4):
        yield from tiny_cases(Cn)
    for name in SHAPES:
        yield shape_case(name)
    yield from edge_cases()


# ------------------------------------------------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("Cn", (2, 3, 4))
def test_tiny_networks_against_the_enumeration(Cn):
    for case in tiny_cases(Cn):
        got = check_case(case)
        assert not np.isnan(got["total"]).any() and not np.isnan(got["post"][:, :case["Jmax"]]).any()


@functools.lru_cache(maxsize=None)
def _shape_result(name):
    case = shape_case(name)
    return case, run_case(case)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_structure_shapes_against_the_float64_lattice(name):
    case, (got, worst, count) = _shape_result(name)
    assert (got["status"] == OK).all() and count > 100, (name, got["status"], count)
    assert worst <= BOUND, (name, worst, BOUND)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_every_slot_sums_to_the_total(name):
    """logsumexp_k post[j, :] == total: every reading picks exactly one entry of slot j."""
    case, (got, _, _) = _shape_result(name)
    for b in range(case["lp"].shape[1]):
        rows = got["post"][b, :int(case["nslots"][b])]
        gap = np.abs(np.logaddexp.reduce(rows, axis=1) - got["total"][b])
        print("%s, utterance %d: max |logsumexp_k post - total| %.3e" % (name, b, gap.max(initial=0.0)))
        assert gap.max(initial=0.0) <= 2 * BOUND, (name, b, gap.max())


@pytest.mark.gpu
def test_edges():
    for case in edge_cases():
        got = check_case(case)
        assert not np.isnan(got["total"]).any() and not np.isnan(got["post"][:, :case["Jmax"]]).any(), case["name"]
        if case["name"] == "classes at -inf":
            assert got["status"].tolist() == [OK, OK, INFEASIBLE] and np.isneginf(got["post"][2, :3]).all()
        if case["name"] == "NaN past len":      # no frames: the all-empty reading alone, its weight the sum of the skips
            skips = case["w"][2, :2, case["blank"]].astype(np.float64)
            assert got["total"][2] == skips[0] + skips[1] and np.isneginf(np.delete(got["post"][2, :2], case["blank"], axis=1)).all()


def variants_case():
    """L = 6, C = 45, T = 30, one posterior matrix three times: the closed network of y, position 2 open, gap 3 open."""
    rs = np.random.default_rng(61)
    T, Cn, L, blank = 30, 45, 6, 0
    y = [7, 7, 19, 3, 44, 12]
    one = ref.posteriors(rs, T, Cn)
    lp = np.stack([one] * 3, axis=1)
    nets = [ref.canonical_network(y, Cn, blank), ref.canonical_network(y, Cn, blank, [2 * 2 + 1]), ref.canonical_network(y, Cn, blank, [2 * 3])]
    w = np.stack(nets)
    return dict(name="variants", lp=lp, lens=[T, T, T], w=w, nslots=[2 * L + 1] * 3, Jmax=2 * L + 1, blank=blank), y


@pytest.mark.gpu
def test_one_open_slot_is_mdd_ctc_variants():
    from tests import test_ctc_variants as tv
    case, y = variants_case()
    got = gpu_confnet(case["lp"], case["lens"], case["w"], case["nslots"], case["Jmax"], case["blank"])
    ids = np.array([y] * 3, np.int32)
    var = tv.gpu_variants(case["lp"], case["lens"], ids, np.array([len(y)] * 3, np.int32), len(y), case["blank"])
    bound = BOUND + tv.BOUND
    assert (got["status"] == OK).all() and (var["status"] == OK).all()
    pairs = [("base", got["total"][:1], var["base"][:1]), ("sub row", got["post"][1, 5], var["sub"][1, 2]), ("ins row", got["post"][2, 6], var["ins"][2, 3])]
    for what, have, want in pairs:
        assert (np.isneginf(have) == np.isneginf(want)).all(), what
        fin = np.isfinite(want)
        err = np.abs(have[fin] - want[fin]).max()
        print("%s: %d finite entries, max |confnet - variants| %.3e (bound %.3e)" % (what, int(fin.sum()), err, bound))
        assert fin.sum() >= 1 and err <= bound, (what, err, bound)
    # a closed slot has one entry: it carries the whole total, every other entry is absent
    closed = got["post"][0]
    for j in range(case["Jmax"]):
        k = case["blank"] if j % 2 == 0 else y[j // 2]
        assert abs(closed[j, k] - got["total"][0]) <= 2 * BOUND and np.isneginf(np.delete(closed[j], k)).all(), j


@functools.lru_cache(maxsize=None)
def _status_batch():
    rs = np.random.default_rng(17)
    T, Cn, blank = 9, 6, 2
    lp, w, nslots = _batch(rs, T, Cn, [_net(rs, J, Cn, blank) for J in (4, 2, 0, 5)], 7)
    w[np.isnan(w)] = 0.5       # rows behind a network: finite here, so that a NaN below is the test's own
    return dict(name="status", lp=lp, lens=[9, 6, 4, 8], w=w, nslots=nslots, Jmax=5, blank=blank, ref="brute")


@pytest.mark.gpu
def test_bad_and_infeasible_rows_leave_their_neighbours_alone():
    case = _status_batch()
    Jmax, blank = case["Jmax"], case["blank"]
    clean = check_case(case)
    assert clean["status"].tolist() == [OK, OK, OK, OK]

    def same_bits(got, b):
        for key in ("total", "post"):
            np.testing.assert_array_equal(bits(got[key][b]), bits(clean[key][b]), err_msg="%s of utterance %d" % (key, b))

    def all_nan(got, b):
        assert np.isnan(got["total"][b]) and np.isnan(got["post"][b, :Jmax]).all() and (got["post"][b, Jmax:] == SENTINEL).all()

    # a NaN weight in utterance 1; a slot without any arc in utterance 3; a NaN behind utterance 0's slots is never read
    w = case["w"].copy()
    w[1, 1, 4] = np.nan
    w[3, 2, :] = NEG
    w[0, 4, 0] = np.nan
    got = gpu_confnet(case["lp"], case["lens"], w, case["nslots"], Jmax, blank)
    assert got["status"].tolist() == [OK, BAD, OK, INFEASIBLE]
    all_nan(got, 1)
    same_bits(got, 0); same_bits(got, 2)
    assert np.isneginf(got["total"][3]) and np.isneginf(got["post"][3, :Jmax]).all() and (got["post"][3, Jmax:] == SENTINEL).all()
    # a +inf weight, a count past Jmax and a negative count around utterance 2
    w = case["w"].copy()
    w[0, 0, 1] = np.inf
    got = gpu_confnet(case["lp"], case["lens"], w, np.array([4, Jmax + 1, 0, -1], np.int32), Jmax, blank)
    assert got["status"].tolist() == [BAD, BAD, OK, BAD]
    for b in (0, 1, 3):
        all_nan(got, b)
    same_bits(got, 2)
    # more frames than len allows for: two equal labels forced into two frames
    w = np.full((1, 2, 3), NEG, np.float32)
    w[0, :, 1] = 0.0
    lp = ref.posteriors(np.random.default_rng(1), 4, 3)[:, None, :]
    got = gpu_confnet(lp, [2], w, [2], 2, 0)
    assert got["status"].tolist() == [INFEASIBLE] and np.isneginf(got["total"][0]) and np.isneginf(got["post"][0]).all()
    got = gpu_confnet(lp, [3], w, [2], 2, 0)
    assert got["status"].tolist() == [OK] and abs(got["total"][0] - float(lp[:3, 0, [1, 0, 1]].astype(np.float64).diagonal().sum())) <= BOUND


@pytest.mark.gpu
def test_workspace_forms_and_repeat_calls_give_the_same_bits():
    import torch
    case = shape_case("C 65 blank 3")
    args = (case["lp"], case["lens"], case["w"], case["nslots"], case["Jmax"], case["blank"])
    first = gpu_confnet(*args)
    for other in (gpu_confnet(*args), gpu_confnet(*args, ws=None)):
        for key in ("total", "post", "status"):
            np.testing.assert_array_equal(bits(other[key]), bits(first[key]), err_msg=key)
    for other in (gpu_confnet(*args, want_post=False), gpu_confnet(*args, ws=None, want_post=False)):
        np.testing.assert_array_equal(bits(other["total"]), bits(first["total"]))
        np.testing.assert_array_equal(other["status"], first["status"])
        assert (other["post"] == SENTINEL).all()
    L_ = _lib()
    T, B, Cn = case["lp"].shape
    need = L_.mdd_ctc_confnet_workspace_bytes(T, B, Cn, case["Jmax"], 1)
    assert need >= 8 * (T - 1) * B * Cn * case["Jmax"] and L_.mdd_ctc_confnet_workspace_bytes(T, B, Cn, case["Jmax"], 0) <= need
    small = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    assert L_.mdd_ctc_confnet(p, T, B, Cn, p, p, case["Jmax"], p, case["Jmax"], case["blank"], p, p, p, C.c_void_p(small.data_ptr()), small.numel(), None) == -1
    assert "workspace" in L_.mdd_last_error().decode()
    torch.cuda.synchronize()
    assert not buf.any()        # refused before any device work


@pytest.mark.gpu
def test_refusals_write_nothing():
    """Every refusal of the header, on device buffers full of zeros: MDD_ERR_ARG, a message that starts with the entry's name and names the
    argument, and nothing written."""
    import torch
    L_ = _lib()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    top = int(L_.mdd_ctc_confnet_max_slots(5))
    for change, name in refusal_cases(p, top):
        a = dict(good_arguments(p), **change)
        assert L_.mdd_ctc_confnet(*[a[k] for k in ORDER], None) == -1, change
        msg = L_.mdd_last_error().decode()
        assert msg.startswith("mdd_ctc_confnet: ") and name in msg, (change, msg)
    torch.cuda.synchronize()
    assert not buf.any()


ORDER = ["logp", "T", "B", "C", "len", "w", "stride", "nslots", "Jmax", "blank", "total", "post", "status", "ws", "ws_bytes"]


def good_arguments(buf):
    return dict(logp=buf, T=10, B=2, C=5, len=buf, w=buf, stride=8, nslots=buf, Jmax=8, blank=0, total=buf, post=buf, status=buf, ws=None, ws_bytes=0)


def refusal_cases(buf, top):
    need = _lib().mdd_ctc_confnet_workspace_bytes(10, 2, 5, 8, 1)
    return [(dict(logp=None), "logp_dev"), (dict(len=None), "len_dev"), (dict(w=None), "w_dev"), (dict(nslots=None), "nslots_dev"),
            (dict(total=None), "total_dev"), (dict(status=None), "status_dev"), (dict(T=0), "T"), (dict(T=-3), "T"), (dict(B=0), "B"),
            (dict(C=0), "C"), (dict(C=257), "C > 256"), (dict(blank=-1), "blank"), (dict(blank=5), "blank"), (dict(Jmax=-1), "Jmax < 0"),
            (dict(Jmax=9), "Jmax > slot_stride"), (dict(stride=top + 1, Jmax=top + 1), "Jmax too long"),
            (dict(ws=buf, ws_bytes=need - 1), "workspace")]
