"""The best reading of an error network on the GPU (mdd_ctc_confnet_best, csrc/ctc_confnet_best.hip) against the float64 references of
tests/confnet_best_reference.py, on the cases of tests/test_ctc_confnet.py: the enumeration of all readings (``brute_best``) on the tiny
and edge networks, the recurrences (``best_f64``, checked against the enumeration on the CPU) at the shapes where the kernel's structure
changes.

Bound on the score: 1e-9 x max(1, |reference|).  Both sides are fp64 sums of fewer than 300 terms of magnitude below 1e2, whose rounding
is some 300 x 1e2 x 2^-53 = 3e-12: the bound leaves orders of magnitude over it.  The reading is pinned by two facts, not by identity with the
reference's (a near tie may fall either way): the score is the optimum, and ``rescore`` of the returned reading and segments -- which
refuses whatever is no reading of the network with a CTC path -- gives the returned score within the same bound."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import confnet_best_reference as best
from tests import confnet_reference as ref
from tests.test_ctc_confnet import SHAPES, edge_cases, shape_case, tiny_cases, _status_batch

pytestmark = pytest.mark.gpu

NEG = -np.inf
OK, INFEASIBLE, BAD = 0, 1, 2
S_SCORE, S_INT = 12345.0, -77
KEYS = ("score", "reading", "status", "path", "seg")


def _lib():
    from ctc_attention_mispronunciation_amd import _lib
    return _lib.lib()


def close(a, b):
    return abs(a - b) <= 1e-9 * max(1.0, abs(b))


def same_bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def gpu_best(lp, lens, w, nslots, Jmax, blank, ws="torch", want_path=True, want_seg=True):
    """mdd_ctc_confnet_best through ctypes on sentinel-filled buffers.  ws: 'torch' (caller workspace of exactly the stated size) or None."""
    import torch
    L_ = _lib()
    T, B, Cn = lp.shape
    stride = w.shape[1]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    lp_d, len_d, ns_d = d(lp.astype(np.float32)), d(np.asarray(lens, np.int32)), d(np.asarray(nslots, np.int32))
    w_d = d(w.astype(np.float32)) if stride else torch.zeros(1, dtype=torch.float32, device="cuda")
    score = torch.full((B,), S_SCORE, dtype=torch.float64, device="cuda")
    reading = torch.full((B, max(stride, 1)), S_INT, dtype=torch.int32, device="cuda")
    status = torch.full((B,), S_INT, dtype=torch.int32, device="cuda")
    path = torch.full((B, T), S_INT, dtype=torch.int32, device="cuda")
    seg = torch.full((B, max(stride, 1), 2), S_INT, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    need = L_.mdd_ctc_confnet_best_workspace_bytes(T, B, Cn, Jmax)
    wsbuf = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda") if ws == "torch" else None
    rc = L_.mdd_ctc_confnet_best(p(lp_d), T, B, Cn, p(len_d), p(w_d), stride, p(ns_d), Jmax, blank, p(score), p(reading), p(status),
                                 p(path) if want_path else None, p(seg) if want_seg else None,
                                 p(wsbuf) if wsbuf is not None else None, need if wsbuf is not None else 0, None)
    assert rc == 0, L_.mdd_last_error().decode()
    torch.cuda.synchronize()
    return dict(score=score.cpu().numpy(), reading=reading.cpu().numpy()[:, :stride], status=status.cpu().numpy(), path=path.cpu().numpy(),
                seg=seg.cpu().numpy()[:, :stride])


def run(case, **kw):
    return gpu_best(case["lp"], case["lens"], case["w"], case["nslots"], case["Jmax"], case["blank"], **kw)


def check_utterance(got, case, b, want):
    """Utterance b of a feasible or infeasible case against the reference score ``want``."""
    name, blank, Jmax = case["name"], case["blank"], case["Jmax"]
    T = case["lp"].shape[0]
    J, Tb = int(case["nslots"][b]), min(max(int(case["lens"][b]), 0), T)
    lp, w = case["lp"][:, b, :], case["w"][b, :J]
    score, reading, seg, path = got["score"][b], got["reading"][b], got["seg"][b], got["path"][b]
    print("%s, utterance %d: J %d, len %d, score %r, reference %r" % (name, b, J, Tb, float(score), want))
    assert (reading[J:Jmax] == -1).all() and (seg[J:Jmax] == -1).all(), (name, b)
    assert (reading[Jmax:] == S_INT).all() and (seg[Jmax:] == S_INT).all(), (name, b)       # rows behind Jmax: untouched
    if np.isneginf(want):
        assert got["status"][b] == INFEASIBLE and np.isneginf(score), (name, b, got["status"][b], score)
        assert (reading[:Jmax] == -1).all() and (seg[:Jmax] == -1).all() and (path == -1).all(), (name, b)
        return
    assert got["status"][b] == OK and np.isfinite(score), (name, b, got["status"][b], score)
    assert close(score, want), (name, b, float(score), want)
    again = best.rescore(lp, Tb, w, blank, reading[:J], seg[:J])
    assert again is not None, (name, b, reading[:J].tolist(), seg[:J].tolist())
    print("    rescore of the returned reading and seg: %r" % again)
    assert close(again, float(score)), (name, b, again, float(score))
    assert (path == best.path_of(seg, J, Tb, T)).all(), (name, b, path.tolist(), seg[:J].tolist())


@functools.lru_cache(maxsize=None)
def _tiny(Cn):
    out = []
    for case in tiny_cases(Cn):
        want = [best.brute_best(case["lp"][:, b, :], int(case["lens"][b]), case["w"][b, :int(case["nslots"][b])], case["blank"])[0]
                for b in range(case["lp"].shape[1])]
        out.append((case, want))
    return out


@pytest.mark.parametrize("Cn", (2, 3, 4))
def test_tiny_networks_against_the_enumeration(Cn):
    for case, want in _tiny(Cn):
        got = run(case)
        for b in range(case["lp"].shape[1]):
            check_utterance(got, case, b, want[b])


@pytest.mark.parametrize("name", SHAPES)
def test_structure_shapes_against_the_float64_recurrences(name):
    case = shape_case(name)
    got = run(case)
    T = case["lp"].shape[0]
    for b in range(case["lp"].shape[1]):
        Tb = min(max(int(case["lens"][b]), 0), T)
        want = best.best_f64(case["lp"][:, b, :], Tb, case["w"][b, :int(case["nslots"][b])], case["blank"])[0]
        assert np.isfinite(want), (name, b)
        check_utterance(got, case, b, want)


def test_edges():
    for case in edge_cases():
        got = run(case)
        T = case["lp"].shape[0]
        for b in range(case["lp"].shape[1]):
            Tb = min(max(int(case["lens"][b]), 0), T)
            want = best.brute_best(case["lp"][:, b, :], Tb, case["w"][b, :int(case["nslots"][b])], case["blank"])[0]
            check_utterance(got, case, b, want)
        assert not np.isnan(got["score"]).any(), case["name"]
        if case["name"] == "classes at -inf":
            assert got["status"].tolist() == [OK, OK, INFEASIBLE]
        if case["name"] == "NaN past len":      # no frames: the all-empty reading alone, its score the sum of the skips
            skips = case["w"][2, :2, case["blank"]].astype(np.float64)
            assert got["score"][2] == skips[0] + skips[1] and (got["reading"][2, :2] == case["blank"]).all() and (got["path"][2] == -1).all()


def test_repeat_rule():
    """C = 3, blank 0, two slots offering only label 1 and no skip: a blank frame must part them."""
    w = np.full((1, 2, 3), NEG, np.float32)
    w[0, :, 1] = 0.0
    lp = ref.posteriors(np.random.default_rng(1), 4, 3)[:, None, :]
    lp[1, 0, :] = np.log(np.array([0.01, 0.98, 0.01], np.float32))       # the posteriors favour label 1 in the middle frame
    got = gpu_best(lp, [2], w, [2], 2, 0)
    assert got["status"].tolist() == [INFEASIBLE] and np.isneginf(got["score"][0])
    assert (got["reading"] == -1).all() and (got["seg"] == -1).all() and (got["path"] == -1).all()
    got = gpu_best(lp, [3], w, [2], 2, 0)
    assert got["status"].tolist() == [OK] and got["reading"][0].tolist() == [1, 1]
    assert got["seg"][0].tolist() == [[0, 1], [2, 3]] and got["path"][0].tolist() == [0, -1, 1, -1]
    assert close(got["score"][0], float(lp[:3, 0, [1, 0, 1]].astype(np.float64).diagonal().sum()))
    # a slot whose own label is the maximum of the slot in front takes the second maximum
    w2 = np.full((1, 2, 3), NEG, np.float32)
    w2[0, 0, 1], w2[0, 0, 2], w2[0, 1, 1] = 0.0, -0.5, 0.0
    lp2 = np.log(np.array([[0.1, 0.8, 0.1], [0.1, 0.8, 0.1]], np.float32))[:, None, :]
    got = gpu_best(lp2, [2], w2, [2], 2, 0)
    assert got["status"].tolist() == [OK] and got["reading"][0].tolist() == [2, 1] and got["seg"][0].tolist() == [[0, 1], [1, 2]]
    assert close(got["score"][0], -0.5 + float(lp2[0, 0, 2]) + float(lp2[1, 0, 1]))


def test_closed_network_is_the_forced_alignment():
    """``canonical_network(y)`` with no open slot has one reading: the score is mdd_ctc_align's on y, to the fp32 accumulation of that
    kernel (one fp32 addition per frame: 2 T 2^-24 relative), the reading y in the position slots and blank in the gaps."""
    from tests.test_ctc_align import gpu_align
    rs = np.random.default_rng(23)
    T, Cn, blank = 25, 45, 0
    ys = [[7, 19, 3, 44, 12], [9, 9]]
    L = 5
    lp = np.stack([ref.posteriors(rs, T, Cn) for _ in ys], axis=1)
    w = np.full((2, 2 * L + 1, Cn), np.nan, np.float32)
    for b, y in enumerate(ys):
        w[b, :2 * len(y) + 1] = ref.canonical_network(y, Cn, blank)
    nslots = [2 * len(y) + 1 for y in ys]
    got = gpu_best(lp, [T, T], w, nslots, 2 * L + 1, blank)
    ids = np.zeros((2, L), np.int32)
    for b, y in enumerate(ys):
        ids[b, :len(y)] = y
    al = gpu_align(lp, [T, T], ids, [len(y) for y in ys], L, blank)
    assert (got["status"] == OK).all() and (al["status"] == OK).all()
    for b, y in enumerate(ys):
        score, want = float(got["score"][b]), float(al["score"][b])
        bound = 2 * T * 2.0 ** -24 * max(1.0, abs(score))
        print("utterance %d: best %r, align %r, bound %.3e" % (b, score, want, bound))
        assert abs(score - want) <= bound, (b, score, want)
        assert got["reading"][b, 1:2 * len(y):2].tolist() == y and (got["reading"][b, 0:2 * len(y) + 1:2] == blank).all(), b
        assert close(best.rescore(lp[:, b], T, w[b, :nslots[b]], blank, got["reading"][b, :nslots[b]], got["seg"][b, :nslots[b]]), score)


def test_bad_and_infeasible_rows_leave_their_neighbours_alone():
    case = _status_batch()
    Jmax, blank = case["Jmax"], case["blank"]
    clean = run(case)
    assert clean["status"].tolist() == [OK, OK, OK, OK]

    def neighbour(got, b):
        for key in KEYS:
            same_bits(got[key][b], clean[key][b], "%s of utterance %d" % (key, b))

    def nothing(got, b):
        assert (got["reading"][b, :Jmax] == -1).all() and (got["seg"][b, :Jmax] == -1).all() and (got["path"][b] == -1).all(), b
        assert (got["reading"][b, Jmax:] == S_INT).all() and (got["seg"][b, Jmax:] == S_INT).all(), b

    # a NaN weight in utterance 1; a slot without any arc in utterance 3; a NaN behind utterance 0's slots is never read
    w = case["w"].copy()
    w[1, 1, 4] = np.nan
    w[3, 2, :] = NEG
    w[0, 4, 0] = np.nan
    got = gpu_best(case["lp"], case["lens"], w, case["nslots"], Jmax, blank)
    assert got["status"].tolist() == [OK, BAD, OK, INFEASIBLE]
    assert np.isnan(got["score"][1]) and np.isneginf(got["score"][3])
    nothing(got, 1); nothing(got, 3)
    neighbour(got, 0); neighbour(got, 2)
    # a +inf weight, a count past Jmax and a negative count around utterance 2
    w = case["w"].copy()
    w[0, 0, 1] = np.inf
    got = gpu_best(case["lp"], case["lens"], w, np.array([4, Jmax + 1, 0, -1], np.int32), Jmax, blank)
    assert got["status"].tolist() == [BAD, BAD, OK, BAD]
    for b in (0, 1, 3):
        assert np.isnan(got["score"][b])
        nothing(got, b)
    neighbour(got, 2)


def test_workspace_forms_optional_outputs_and_repeat_calls_give_the_same_bits():
    import torch
    case = shape_case("C 65 blank 3")
    first = run(case)
    for other in (run(case), run(case, ws=None)):
        for key in KEYS:
            same_bits(other[key], first[key], key)
    for kw, untouched in ((dict(want_path=False), ("path",)), (dict(want_seg=False), ("seg",)), (dict(want_path=False, want_seg=False), ("path", "seg"))):
        other = run(case, **kw)
        for key in KEYS:
            if key in untouched:
                assert (other[key] == S_INT).all(), (kw, key)
            else:
                same_bits(other[key], first[key], "%s with %s" % (key, kw))
    L_ = _lib()
    T, B, Cn = case["lp"].shape
    need = L_.mdd_ctc_confnet_best_workspace_bytes(T, B, Cn, case["Jmax"])
    assert need > 1
    small = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    assert L_.mdd_ctc_confnet_best(p, T, B, Cn, p, p, case["Jmax"], p, case["Jmax"], case["blank"], p, p, p, p, p,
                                   C.c_void_p(small.data_ptr()), small.numel(), None) == -1
    assert "workspace" in L_.mdd_last_error().decode()
    torch.cuda.synchronize()
    assert not buf.any()        # refused before any device work


ORDER = ["logp", "T", "B", "C", "len", "w", "stride", "nslots", "Jmax", "blank", "score", "reading", "status", "path", "seg", "ws", "ws_bytes"]


def test_refusals_write_nothing():
    """Every refusal of mdd_ctc_confnet, and the outputs of this entry, on device buffers full of zeros: MDD_ERR_ARG, a message that
    starts with the entry's name and names the argument, and nothing written."""
    import torch
    L_ = _lib()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    top = int(L_.mdd_ctc_confnet_max_slots(5))
    good = dict(logp=p, T=10, B=2, C=5, len=p, w=p, stride=8, nslots=p, Jmax=8, blank=0, score=p, reading=p, status=p, path=p, seg=p, ws=None,
                ws_bytes=0)
    need = L_.mdd_ctc_confnet_best_workspace_bytes(10, 2, 5, 8)
    cases = [(dict(logp=None), "logp_dev"), (dict(len=None), "len_dev"), (dict(w=None), "w_dev"), (dict(nslots=None), "nslots_dev"),
             (dict(score=None), "score_dev"), (dict(reading=None), "reading_dev"), (dict(status=None), "status_dev"), (dict(T=0), "T"),
             (dict(T=-3), "T"), (dict(B=0), "B"), (dict(C=0), "C"), (dict(C=257), "C > 256"), (dict(blank=-1), "blank"), (dict(blank=5), "blank"),
             (dict(Jmax=-1), "Jmax < 0"), (dict(Jmax=9), "Jmax > slot_stride"), (dict(stride=top + 1, Jmax=top + 1), "Jmax too long"),
             (dict(ws=p, ws_bytes=need - 1), "workspace")]
    for change, name in cases:
        a = dict(good, **change)
        assert L_.mdd_ctc_confnet_best(*[a[k] for k in ORDER], None) == -1, change
        msg = L_.mdd_last_error().decode()
        assert msg.startswith("mdd_ctc_confnet_best: ") and name in msg, (change, msg)
    torch.cuda.synchronize()
    assert not buf.any()


def test_python_entries_against_the_references():
    """hip_model.ctc_confnet_best and ctcDecoder.joint_diagnosis at T = 25, C = 45, L = 5, B = 3: the score and the reading as above, the
    posterior against float64: the reading's prior + CPU ctc_loss in double of its labels - lattice_f64's total, within 1e-4."""
    import torch
    from ctc_attention_mispronunciation_amd.hip_model import ctc_confnet_best
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import error_network, joint_diagnosis
    rs = np.random.default_rng(41)
    T, Cn, L, B, blank, P = 25, 45, 5, 3, 0, 0.05
    lp = np.stack([ref.posteriors(rs, T, Cn) for _ in range(B)], axis=1)
    ids = rs.integers(1, Cn, size=(B, L)).astype(np.int32)
    nids = np.array([5, 3, 4], np.int32)
    lens = [25, 20, 25]
    for b in range(B):                      # the frames lean towards the canonical ids, so that the best reading keeps most of them
        for i in range(int(nids[b])):
            lp[3 * i + 1:3 * i + 3, b, ids[b, i]] += 6.0
    lp = (lp - np.log(np.exp(lp.astype(np.float64)).sum(axis=-1, keepdims=True))).astype(np.float32)
    w_t, ns_t = error_network(torch.from_numpy(ids), torch.from_numpy(nids), Cn, blank, P)
    w, nslots = w_t.numpy(), ns_t.numpy()
    r = ctc_confnet_best(torch.from_numpy(lp).cuda(), lens, w_t, ns_t, blank=blank)
    got = dict(score=r.score.cpu().numpy(), reading=r.reading.cpu().numpy(), status=r.status.cpu().numpy(), path=r.path.cpu().numpy(),
               seg=r.seg.cpu().numpy())
    assert got["reading"].dtype == np.int32 and got["seg"].shape == (B, 2 * L + 1, 2) and got["path"].shape == (B, T)
    out = joint_diagnosis(torch.from_numpy(lp).cuda(), lens, torch.from_numpy(ids), torch.from_numpy(nids), blank, error_prior=P)
    kept = 0
    for b in range(B):
        J, n = int(nslots[b]), int(nids[b])
        want = best.best_f64(lp[:, b], lens[b], w[b, :J], blank)[0]
        assert got["status"][b] == OK and close(got["score"][b], want), (b, got["score"][b], want)
        again = best.rescore(lp[:, b], lens[b], w[b, :J], blank, got["reading"][b, :J], got["seg"][b, :J])
        assert again is not None and close(again, got["score"][b]), b
        assert (got["path"][b] == best.path_of(got["seg"][b], J, lens[b], T)).all() and (got["reading"][b, J:] == -1).all(), b
        positions, gaps, score, posterior = out[b]
        assert len(positions) == n and len(gaps) == n + 1 and score == got["score"][b], b
        slots = [None] * J
        slots[1::2], slots[0::2] = positions, gaps
        assert [s[0] for s in slots] == got["reading"][b, :J].tolist() and [list(s[1:]) for s in slots] == got["seg"][b, :J].tolist(), b
        labels = [k for k, _, _ in slots if k != blank]
        prior = sum(float(np.float64(w[b, j, k])) for j, (k, _, _) in enumerate(slots))
        nll = torch.nn.functional.ctc_loss(torch.from_numpy(lp[:lens[b], b:b + 1]).double(), torch.tensor([labels], dtype=torch.long),
                                           torch.tensor([lens[b]]), torch.tensor([len(labels)]), blank=blank, reduction="sum")
        total = ref.lattice_f64(lp[:, b], lens[b], w[b, :J], blank)
        want_p = float(np.exp(prior - float(nll) - total))
        print("utterance %d: reading %s, posterior %r, float64 %r" % (b, [s[0] for s in slots], posterior, want_p))
        assert 0.0 < posterior <= 1.0 and abs(posterior - want_p) <= 1e-4, (b, posterior, want_p)
        kept += sum(p[0] == int(ids[b, i]) for i, p in enumerate(positions))
    assert kept >= 6, "the posteriors lean towards the canonical ids: most positions are kept"
    with pytest.raises(TypeError):
        joint_diagnosis(torch.from_numpy(lp).cuda(), lens, torch.from_numpy(ids), torch.from_numpy(nids), blank)
    with pytest.raises(ValueError, match="error_prior"):
        joint_diagnosis(torch.from_numpy(lp).cuda(), lens, torch.from_numpy(ids), torch.from_numpy(nids), blank, error_prior=1.0)
    # ids that are no targets: no result for that utterance, the others unchanged
    bad = ids.copy()
    bad[1, 0] = blank
    out2 = joint_diagnosis(torch.from_numpy(lp).cuda(), lens, torch.from_numpy(bad), torch.from_numpy(nids), blank, error_prior=P)
    assert out2[1] is None and out2[0] == out[0] and out2[2] == out[2]
