"""The host side of mdd_ctc_nbest (csrc/ctc_nbest.hip), without a GPU.

  * the two symbols are declared, listed and exported;
  * every refusal of the entry: MDD_ERR_ARG before any device work (the pointers are fake and never dereferenced), the message starting
    with the entry's name and naming the argument;
  * mdd_ctc_nbest_fits on both sides of the T bound, and csrc/plan.h's ctc_nbest_plan with the host compiler (tests/ctc_nbest_cases.py's
    driver): the library's answers are the plan's, the LDS of every accepted shape fits a CU, NL is ctc_labels_per_lane, the grid covers
    N exactly;
  * BeamDecoder.nbest_loglik's routing: one ctc_nbest call where the shape fits, the loop over ctc_loss where it does not;
  * the cases' own condition: at least half of the (n, b) pairs of each are finite under the float64 reference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import ctc_nbest_cases as cc
from tests.helpers import GOLD, ROOT

MDD_ERR_ARG = -1
_FAKE = 4096      # a non-NULL value for pointers that must never be dereferenced: every call below is refused on the host
KB = 1024


def _L():
    from ctc_attention_mispronunciation_amd import _lib
    return _lib.lib()


def test_symbols_are_declared_listed_and_exported():
    from ctc_attention_mispronunciation_amd import _lib
    header = open(os.path.join(ROOT, "include", "mdd_hip.h")).read()
    assert re.search(r"\bint mdd_ctc_nbest\s*\(", header) and re.search(r"\bint mdd_ctc_nbest_fits\s*\(", header)
    for name in ("mdd_ctc_nbest", "mdd_ctc_nbest_fits"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
    assert _lib.lib().mdd_version() == 100


# ----------------------------------------------------------------------------------------------------------------- refusals
def _args(**over):
    a = dict(logp=_FAKE, T=40, B=3, C=45, len=_FAKE, ids=_FAKE, pitch=40, nids=_FAKE, N=10, max_len=10, blank=0, loglik=_FAKE)
    a.update(over)
    vp = C.c_void_p
    return (vp(a["logp"]), a["T"], a["B"], a["C"], vp(a["len"]), vp(a["ids"]), a["pitch"], vp(a["nids"]), a["N"], a["max_len"], a["blank"],
            vp(a["loglik"]), None)


_REFUSALS = [
    (dict(logp=None), "logp_dev"), (dict(len=None), "len_dev"), (dict(ids=None), "ids_dev"), (dict(nids=None), "nids_dev"),
    (dict(loglik=None), "loglik_dev"),
    (dict(N=0), "N<=256"), (dict(N=257), "N<=256"), (dict(B=0), "<=B"), (dict(C=1), "C<=256"), (dict(C=257), "C<=256"), (dict(T=0), "T < 1"),
    (dict(blank=-1), "blank"), (dict(blank=45), "blank"),
    (dict(max_len=-1), "max_len"), (dict(max_len=256, pitch=300), "max_len"), (dict(max_len=41, pitch=40), "max_len"),
    (dict(T=660), "T too long"), (dict(T=117, C=256, blank=0), "T too long"),
]


@pytest.mark.parametrize("over,needle", _REFUSALS, ids=["_".join("%s=%s" % kv for kv in o.items()) for o, _ in _REFUSALS])
def test_bad_arguments_are_refused_on_the_host(over, needle):
    L = _L()
    assert L.mdd_ctc_nbest(*_args(**over)) == MDD_ERR_ARG
    msg = L.mdd_last_error().decode()
    assert msg.startswith("mdd_ctc_nbest") and needle in msg, msg


def test_a_refused_shape_is_one_the_fits_query_refuses():
    L = _L()
    assert L.mdd_ctc_nbest_fits(659, 45, 10) == 1 and L.mdd_ctc_nbest_fits(660, 45, 10) == 0
    assert L.mdd_ctc_nbest(*_args(T=660)) == MDD_ERR_ARG and "LDS" in L.mdd_last_error().decode()


# -------------------------------------------------------------------------------------------------- the fits query and the plan
def test_fits_query_and_plan_on_the_host():
    from ctc_attention_mispronunciation_amd import hip_model
    L = _L()
    # both sides of the T bound: 4 T C <= 116 KiB, the block of a shape mdd_ctc_loss still gives its wave kernel (csrc/plan.h)
    for Cn, tmax in ((45, 116 * KB // (4 * 45)), (256, 116 * KB // (4 * 256))):
        for max_len in (0, 64, 255):
            assert L.mdd_ctc_nbest_fits(tmax, Cn, max_len) == 1 and L.mdd_ctc_nbest_fits(tmax + 1, Cn, max_len) == 0, (Cn, max_len)
        assert L.mdd_ctc_nbest_fits(tmax, Cn, 256) == 0 and L.mdd_ctc_nbest_fits(1, Cn, 256) == 0
    assert (116 * KB // (4 * 45), 116 * KB // (4 * 256)) == (659, 116)
    assert hip_model.ctc_nbest_fits(659, 45, 255) is True and hip_model.ctc_nbest_fits(660, 45, 255) is False
    assert hip_model.ctc_nbest_fits(40, 45, 256) is False
    # the plan, written out, over every probed shape; then the library against the plan's own answers
    r = subprocess.run([cc.plan_driver()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "; 0 mismatch(es)" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"accepted (\d+) shapes; largest LDS of a workgroup: (\d+) bytes", r.stdout)
    assert int(m.group(1)) > 10000 and int(m.group(2)) <= 116 * KB <= 160 * KB
    probes = [tuple(int(v) for v in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("fits ")]
    assert len(probes) == 150 and {p[3] for p in probes} == {0, 1}
    for T, Cn, max_len, want in probes:
        assert L.mdd_ctc_nbest_fits(T, Cn, max_len) == want, (T, Cn, max_len)
    tmax = dict(tuple(int(v) for v in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("tmax "))
    assert tmax[45] == 659 and tmax[256] == 116
    # every shape mdd_ctc_nbest_fits takes is one mdd_ctc_loss gives ctc_wave_kernel (tests/ctc_loss_cases.py restates its rule)
    from tests import ctc_loss_cases as lc
    for Cn in (2, 45, 101, 256):
        for max_len in (1, 63, 64, 127, 128, 255):
            T = 116 * KB // (4 * Cn)
            assert L.mdd_ctc_nbest_fits(T, Cn, max_len) == 1 and lc.expected_form(T, Cn, max_len) == "wave%d" % lc.labels_per_lane(max_len)


def test_plan_counts_through_the_cases_helper():
    p = cc.plan(40, 3, 45, 35, 10)
    assert p.fits == 1 and p.NL == 1 and p.smem == 4 * 40 * 45 and p.groups == -(-35 // p.hyps_per_block) and p.waves >= 1
    assert cc.plan(300, 2, 45, 3, 64).NL == 2 and cc.plan(300, 2, 45, 3, 128).NL == 4 and cc.plan(300, 2, 45, 3, 255).NL == 4
    assert cc.plan(660, 1, 45, 3, 10).fits == 0 and cc.plan(300, 2, 45, 3, 256).fits == 0
    # the shapes of the sweep (profiles/ctc_nbest_notes.txt): a SIMD per scan while the device has them, ten ranks a workgroup beyond
    assert [cc.plan(250, B, 45, N, 64).hyps_per_block for B, N in ((64, 1), (64, 10), (512, 10), (64, 200))] == [1, 4, 10, 10]
    assert cc.plan(600, 64, 45, 200, 255).hyps_per_block == 10 and cc.plan(600, 1, 45, 8, 255).hyps_per_block == 8


# ------------------------------------------------------------------------------------------------------------------ routing
def _decoder(beam=10):
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    return BeamDecoder(synth.phone_table_41(), beam_width=beam, blank_index=0, space_idx=-1, lm_path=os.path.join(GOLD, "lm_synth45.arpa"), lm_alpha=0.0)


@pytest.mark.parametrize("T,pitch,max_len,fits", [(40, 40, 10, True), (40, 40, None, True), (659, 16, 12, True), (660, 16, 12, False),
                                                  (300, 300, 256, False), (300, 300, 255, True), (300, 300, None, False)])
def test_nbest_loglik_routes_on_the_fits_query(monkeypatch, T, pitch, max_len, fits):
    """hip_model.ctc_nbest and hip_model.ctc_loss replaced by counters (host tensors, no device): one call of the first where the shape
    fits, N calls of the second where it does not; the values come back as float64 [N, B], rounded through fp32 and negated."""
    from ctc_attention_mispronunciation_amd import hip_model
    from ctc_attention_mispronunciation_amd.utils import ctcDecoder
    N, B, Cn = 5, 3, 45
    calls = {"nbest": [], "loss": []}

    def fake_nbest(logp, lens, ids, nids, blank=0, max_len=None):
        calls["nbest"].append((tuple(ids.shape), max_len, blank))
        return torch.full((ids.shape[0], logp.shape[1]), -1.0 - 2.0 ** -30, dtype=torch.float64)

    def fake_loss(logp, targets, in_len, tgt_len, blank=0, want_grad=True):
        calls["loss"].append((tuple(targets.shape), want_grad, blank))
        return torch.full((logp.shape[1],), 1.0, dtype=torch.float32), None

    def host_posteriors(prob_tensor, frame_seq_len):
        return prob_tensor, prob_tensor.shape[0], prob_tensor.shape[1], prob_tensor.shape[2], torch.tensor(frame_seq_len, dtype=torch.int32)

    monkeypatch.setattr(hip_model, "ctc_nbest", fake_nbest)
    monkeypatch.setattr(hip_model, "ctc_loss", fake_loss)
    monkeypatch.setattr(ctcDecoder, "_posteriors_and_lens", host_posteriors)
    ids, nids = torch.zeros((N, B, pitch), dtype=torch.int32), torch.ones((N, B), dtype=torch.int32)
    ll = _decoder().nbest_loglik(torch.zeros((T, B, Cn)), [T] * B, ids, nids, max_len=max_len)
    assert ll.dtype == np.float64 and ll.shape == (N, B) and (ll == -1.0).all()          # -(1 + 2^-30) through fp32 is -1
    width = pitch if max_len is None else max_len
    if fits:
        assert calls["loss"] == [] and calls["nbest"] == [((N, B, pitch), width, 0)]
    else:
        assert calls["nbest"] == [] and calls["loss"] == [((B, width), False, 0)] * N


# ---------------------------------------------------------------------------------------------------------------- the cases
def test_at_least_half_of_each_case_is_finite_under_the_reference():
    cases = [cc.ragged("peaky"), cc.ragged("dense"), cc.ragged("dense", C=2, blank=1), cc.ragged("dense", C=256, blank=100),
             cc.ragged("peaky", blank=44)] + [cc.form(n) for n in (63, 64, 127, 128, 255)]
    for c in cases:
        ref = cc.reference(c.name, min(35, c.ids.shape[0]))
        assert not np.isnan(ref).any() and np.isfinite(ref).mean() >= 0.5, (c.name, np.isfinite(ref).mean())
        assert (c.nids <= c.max_len).all() and (c.ids[..., :c.max_len] != c.blank).any()
        for b, need in enumerate(c.lens):          # the rule the cases were drawn by: frames for every label and a blank between any two
            if c.name.startswith("ragged"):
                assert need >= 2 * int(c.nids[:, b].max()) + 1, (c.name, b)
