"""The float64 references of the error-network CTC against the enumeration of all readings, and the host side of the feature: the error
network's rows, the tuples of ``joint_phoneme_posteriors``, the flag errors, the exported symbols, the argument refusals.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import confnet_reference as ref
from tests.helpers import ROOT

NEG = -np.inf
SYMBOLS = ("mdd_ctc_confnet", "mdd_ctc_confnet_workspace_bytes", "mdd_ctc_confnet_max_slots")


def test_references_match_the_enumeration_in_float64():
    """lattice_f64 / marginals_f64 (and the forward / backward restatement) against brute on seeded tiny networks: C 2..4, T 0..6, J 0..5,
    absent arcs, every blank index.  -inf patterns identical; finite entries within 1e-9 (seen: 4e-15)."""
    rs = np.random.default_rng(1)
    n = n_inf = 0
    blanks = set()
    for case in range(140):
        Cn, T, J = int(rs.integers(2, 5)), int(rs.integers(0, 7)), int(rs.integers(0, 6))
        blank = case % Cn
        blanks.add((Cn, blank))
        lp = np.log(rs.dirichlet(np.ones(Cn), size=max(T, 1)))
        w = ref.random_network(rs, J, Cn)
        total, post = ref.brute(lp, T, w, blank)
        fb_total, fb_post = ref.forward_backward_f64(lp, T, w, blank)
        pairs = [("lattice", [ref.lattice_f64(lp, T, w, blank)], [total]), ("marginals", ref.marginals_f64(lp, T, w, blank), post),
                 ("sweep total", [fb_total], [total]), ("sweep marginals", fb_post, post)]
        for what, have, want in pairs:
            have, want = np.asarray(have, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
            assert (np.isneginf(have) == np.isneginf(want)).all() and not np.isnan(have).any(), (case, what, have, want)
            fin = np.isfinite(want)
            assert np.abs(have[fin] - want[fin]).max(initial=0.0) < 1e-9, (case, what)
        if np.isfinite(total) and J:          # every reading picks one entry of every slot
            assert np.abs(np.logaddexp.reduce(post, axis=1) - total).max() < 1e-9
        n += post.size
        n_inf += int(np.isneginf(post).sum())
    assert n > 1000 and 100 < n_inf < n - 300 and len(blanks) == 9       # both kinds of outcome, every blank index


def test_sampled_marginals_are_the_full_ones():
    rs = np.random.default_rng(2)
    lp, w = ref.posteriors(rs, 5, 4), ref.random_network(rs, 4, 4, 0.1)
    full = ref.marginals_f64(lp, 5, w, 1)
    ent = [(3, 1), (0, 0), (2, 3), (0, 0)]
    np.testing.assert_array_equal(ref.marginals_f64(lp, 5, w, 1, ent), np.array([full[j, k] for j, k in ent]))
    batch = ref.lattice_f64(lp, 5, np.stack([w, w[::-1].copy()]), 1)
    assert batch[0] == ref.lattice_f64(lp, 5, w, 1) and batch[1] == ref.lattice_f64(lp, 5, w[::-1].copy(), 1)


def test_closed_network_is_ctc_and_one_open_slot_is_a_variant_row():
    """The consequences the GPU test pins against mdd_ctc_variants, here in float64 against its brute force."""
    from tests.test_ctc_variants import brute as ctc_brute, variant_target
    rs = np.random.default_rng(3)
    Cn, T, blank, y = 5, 8, 2, [0, 0, 4, 1]
    lp = ref.posteriors(rs, T, Cn)
    base = ctc_brute(lp, T, [y], blank)[0]
    assert abs(ref.lattice_f64(lp, T, ref.canonical_network(y, Cn, blank), blank) - base) < 1e-12
    for kind, pos, slot in (("s", 1, 3), ("s", 3, 7), ("i", 0, 0), ("i", 4, 8), ("i", 2, 4)):
        post = ref.marginals_f64(lp, T, ref.canonical_network(y, Cn, blank, [slot]), blank)[slot]
        want = ctc_brute(lp, T, [variant_target(y, blank, kind, pos, k) for k in range(Cn)], blank)
        assert (np.isneginf(post) == np.isneginf(want)).all(), (kind, pos)
        fin = np.isfinite(want)
        assert np.abs(post[fin] - want[fin]).max() < 1e-12, (kind, pos)


def test_error_network_rows():
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import error_network
    ids = torch.tensor([[3, 1, 3], [2, 0, 0]], dtype=torch.int32)
    nids = torch.tensor([3, 1], dtype=torch.int32)
    w, nslots = error_network(ids, nids, 5, blank=4)
    assert w.dtype == torch.float32 and tuple(w.shape) == (2, 7, 5) and nslots.tolist() == [7, 3] and nslots.dtype == torch.int32
    assert not w.any()                                # the uniform prior: every entry of every slot at weight 0
    P = 0.2
    w, nslots = error_network(ids, nids, 5, blank=4, error_prior=P)
    keep, err = np.float32(math.log(1 - P)), np.float32(math.log(P / 4))
    w = w.numpy()
    for b, y in enumerate(([3, 1, 3], [2])):
        for g in range(len(y) + 1):
            assert w[b, 2 * g, 4] == keep and (np.delete(w[b, 2 * g], 4) == err).all()
        for i, k in enumerate(y):
            assert w[b, 2 * i + 1, k] == keep and (np.delete(w[b, 2 * i + 1], k) == err).all()
    assert nslots.tolist() == [7, 3]
    assert abs(np.exp(w[0, 1].astype(np.float64)).sum() - 1.0) < 1e-6 and abs(np.exp(w[0, 0].astype(np.float64)).sum() - 1.0) < 1e-6
    w0, n0 = error_network(torch.zeros((2, 0), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 3)
    assert tuple(w0.shape) == (2, 1, 3) and n0.tolist() == [1, 1] and not w0.any()
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="error_prior"):
            error_network(ids, nids, 5, 4, bad)
    with pytest.raises(ValueError, match="blank"):
        error_network(ids, nids, 5, 5)


def test_joint_posterior_tuples_on_canned_marginals():
    """The tuple assembly of joint_phoneme_posteriors: positions from the odd slots, gaps from the even ones, exp(post - total)."""
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import _posterior_tuples
    blank, Cn = 0, 4
    ids = np.array([[2, 1], [3, 0]])
    n = np.array([2, 1])
    total = np.array([-3.0, -1.0])
    p = np.zeros((2, 5, Cn))
    p[0] = [[0.7, 0.1, 0.2, 0.0], [0.25, 0.125, 0.5, 0.125], [1.0, 0.0, 0.0, 0.0], [0.5, 0.25, 0.0, 0.25], [0.9, 0.0, 0.0, 0.1]]
    p[1, :3] = [[0.5, 0.0, 0.5, 0.0], [0.0, 0.0, 0.0, 1.0], [0.25, 0.25, 0.25, 0.25]]
    with np.errstate(divide="ignore"):
        post = np.log(p) + total[:, None, None]
    out = _posterior_tuples(post, total, np.array([0, 0]), ids, n, blank)

    def same(have, want):
        assert len(have) == len(want)
        for h, w_ in zip(have, want):
            assert len(h) == len(w_) and all(type(a) is type(b) for a, b in zip(h, w_)), (h, w_)
            assert all(a == b if isinstance(b, int) else abs(a - b) < 1e-14 for a, b in zip(h, w_)), (h, w_)

    positions, gaps = out[0]
    same(positions, [(0.5, 0.25, 1, 0.125), (0.25, 0.5, 3, 0.25)])          # (p_correct, p_deleted, alt_id, p_alt); ties: the lower id
    same(gaps, [(2, 0.2), (1, 0.0), (3, 0.1)])
    positions, gaps = out[1]
    same(positions, [(1.0, 0.0, 1, 0.0)])
    same(gaps, [(2, 0.5), (1, 0.25)])
    assert _posterior_tuples(post, total, np.array([1, 2]), ids, n, blank) == [None, None]


def test_flag_errors_exit_with_status_2(capsys):
    from ctc_attention_mispronunciation_amd import infer as infer_cli
    from ctc_attention_mispronunciation_amd import infer_core
    base = ["--conf", "no-such-conf.yaml", "--wav_transcript_path", "no-such-folder"]
    for extra in (["--error_prior", "0.1"], ["--joint_posteriors", "--error_prior", "0"], ["--joint_posteriors", "--error_prior", "1"],
                  ["--joint_posteriors", "--error_prior", "-0.5"], ["--joint_posteriors", "--error_prior", "1.5"],
                  ["--joint_posteriors", "--error_prior", "nan"]):
        with pytest.raises(SystemExit) as e:
            infer_cli.main(base + extra)
        assert e.value.code == 2, extra
        assert "--error_prior" in capsys.readouterr().err
    args = infer_cli.parse_args(base + ["--joint_posteriors", "--error_prior", "0.25"])
    assert args.joint_posteriors and args.error_prior == 0.25
    args = infer_cli.parse_args(base)
    assert not args.joint_posteriors and args.error_prior is None
    for kw in (dict(error_prior=0.1), dict(joint_posteriors=True, error_prior=1.0)):
        with pytest.raises(ValueError, match="error_prior"):
            infer_core.infer(None, None, [], None, None, None, None, None, False, **kw)


def test_symbols_declared_listed_and_exported():
    from ctc_attention_mispronunciation_amd import _lib
    header = open(os.path.join(ROOT, "include", "mdd_hip.h")).read()
    L_ = _lib.lib()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.EXPORTS and hasattr(L_, name), name
    assert L_.mdd_ctc_confnet_max_slots(45) >= 129              # a 64-phoneme canonical
    assert L_.mdd_ctc_confnet_max_slots(1) == -1 and L_.mdd_ctc_confnet_max_slots(257) == -1 and L_.mdd_ctc_confnet_max_slots(0) == -1
    tops = [L_.mdd_ctc_confnet_max_slots(c) for c in (2, 45, 64, 65, 256)]
    assert tops == sorted(tops, reverse=True) and tops[-1] >= 1
    assert L_.mdd_ctc_confnet_workspace_bytes(250, 64, 45, 129, 1) >= 8 * 249 * 64 * 45 * 129
    assert L_.mdd_ctc_confnet_workspace_bytes(250, 64, 45, 129, 0) <= L_.mdd_ctc_confnet_workspace_bytes(250, 64, 45, 129, 1)


def test_confnet_rejects_bad_arguments_before_device_work():
    """Every argument error returns MDD_ERR_ARG and names the argument; host addresses stand in for device buffers, none is used."""
    from ctc_attention_mispronunciation_amd import _lib
    from tests.test_ctc_confnet import ORDER, good_arguments, refusal_cases
    L_ = _lib.lib()
    host = np.zeros(64, np.float32)
    buf = C.c_void_p(host.ctypes.data)
    for change, name in refusal_cases(buf, int(L_.mdd_ctc_confnet_max_slots(5))):
        a = dict(good_arguments(buf), **change)
        assert L_.mdd_ctc_confnet(*[a[k] for k in ORDER], None) == -1, change
        msg = L_.mdd_last_error().decode()
        assert msg.startswith("mdd_ctc_confnet: ") and name in msg, (change, msg)
    assert not host.any()
