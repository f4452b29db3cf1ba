"""The text encoder's input projection as a gather from the weight set's table of projected embedding rows (embed_index_kernel,
gather_rows_kernel) against the per-call form it replaces (MDD_TEXT_PROJ=gemm: embed_kernel, then the projection GEMM): the table's rows
are made by the same GEMM from the same operands, so the log-probs and the "text" and "key" taps must agree bit for bit.  No tolerance
anywhere in this file: every comparison is on int32 bit patterns."""
import os
import subprocess

import numpy as np
import pytest
import torch

from ctc_attention_mispronunciation_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 38
GEOMS = {"ref": synth.REFERENCE, "ref256": synth.REFERENCE_256, "tiny": synth.TINY}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _model(geom, sd, precision, text_proj=None):
    """A model created with MDD_TEXT_PROJ as given (the switch is read when a model is created)."""
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    saved = os.environ.pop("MDD_TEXT_PROJ", None)
    try:
        if text_proj:
            os.environ["MDD_TEXT_PROJ"] = text_proj
        return HipModel(geom, sd, precision=precision)
    finally:
        os.environ.pop("MDD_TEXT_PROJ", None)
        if saved is not None:
            os.environ["MDD_TEXT_PROJ"] = saved


_PAIRS = {}


def _pair(name, precision, seed=83):
    """(table model, per-call GEMM model) of one geometry, arithmetic and weight set, shared by the cases of this file."""
    key = (name, precision, seed)
    if key not in _PAIRS:
        geom = synth.Geometry(**GEOMS[name])
        sd = synth.synth_state_dict(geom, seed=seed)
        _PAIRS[key] = (geom, _model(geom, sd, precision), _model(geom, sd, precision, "gemm"))
    return _PAIRS[key]


def _ids(geom, B, L, start=0):
    """Canonical ids [B, L]: the rows 1 .. emb_rows - 1 in turn (every row within emb_rows - 1 positions), the second position of an
    utterance repeating its first, and from L = 3 on id 0 padding at the end of every utterance but the first."""
    n = geom.emb_rows - 1
    x1 = (1 + (start + np.arange(B * L, dtype=np.int64)) % n).reshape(B, L)
    if L >= 2:
        x1[:, 1] = x1[:, 0]
    if L >= 3:
        x1[1:, -(1 + L // 4):] = 0
        x1[0, -1] = 0
    return x1


def _run(m, x, x1):
    out = m.forward(_cuda(x), _cuda(x1), sync_errors=True).clone()
    return out, m.tap("text").clone(), m.tap("key").clone()


def _assert_same(got, want):
    for g, w, what in zip(got, want, ("logp", "text", "key")):
        assert g.shape == w.shape and torch.equal(_bits(g), _bits(w)), what


def test_ids_cover_every_row():
    """The id pattern of the cases below: at 17 x 40 and 17 x 65 one call alone holds every row 0 .. 43, a repeat and padding."""
    geom = synth.Geometry(**synth.REFERENCE)
    for B, L in [(17, 40), (17, 65), (3, 40)]:
        x1 = _ids(geom, B, L)
        assert set(x1.ravel().tolist()) == set(range(geom.emb_rows)), (B, L)
        assert (x1[:, 1] == x1[:, 0]).all() and (x1[:, -1] == 0).all()
    union = set()
    for B in (1, 3, 17):
        for L in (1, 7, 40, 65):
            union |= set(_ids(geom, B, L, start=B + L).ravel().tolist())
    assert union == set(range(geom.emb_rows))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32x6", "f32"])
@pytest.mark.parametrize("L", [1, 7, 40, 65])
@pytest.mark.parametrize("B", [1, 3, 17])
def test_text_table_equals_per_call_projection(B, L, precision):
    geom, new, old = _pair("ref", precision)
    assert new.precision == old.precision == precision
    x, _, _, _ = synth.synth_batch(geom, B=B, T=T, L=L, seed=B + L, ragged=False)
    x1 = _ids(geom, B, L, start=B + L)
    got, want = _run(new, x, x1), _run(old, x, x1)
    assert got[1].numel() == L * B * 2 * geom.hidden
    _assert_same(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision,want_mode,L", [("ref256", "f32x6", "f32x6", 40), ("tiny", "f32x6", "f32", 7)])
def test_text_table_other_geometries(name, precision, want_mode, L):
    """H = 256; and the tiny geometry, whose embedding width (12) has no f32x6 planes: the mode falls back to f32 and so does the table."""
    geom, new, old = _pair(name, precision)
    assert new.precision == old.precision == want_mode
    B = 3
    x, _, _, _ = synth.synth_batch(geom, B=B, T=T, L=L, seed=5, ragged=False)
    x1 = _ids(geom, B, L)
    assert set(x1.ravel().tolist()) == set(range(geom.emb_rows))
    _assert_same(_run(new, x, x1), _run(old, x, x1))


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [44, -1, 1 << 40])
def test_text_table_out_of_range_id_raises_on_both_paths(bad):
    geom, new, old = _pair("ref", "f32x6")
    B, L = 3, 7
    x, _, _, _ = synth.synth_batch(geom, B=B, T=T, L=L, seed=1, ragged=False)
    x1 = _ids(geom, B, L)
    x1[2, 3] = bad
    msgs = []
    for m in (new, old):
        with pytest.raises(IndexError) as e:
            m.forward(_cuda(x), _cuda(x1), sync_errors=True)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] == "index out of range in self"
    x1[2, 3] = 5   # the flag is cleared by the raise: the next call is an ordinary one, on both paths
    _assert_same(_run(new, x, x1), _run(old, x, x1))


@pytest.mark.gpu
def test_text_table_fused_batches_through_graph_replays():
    """Batches with L_g = 1, 9 and 40 in one fused launch sequence: the capture, then three replays of the captured graph."""
    geom, new, old = _pair("ref", "f32x6")
    shapes = [(4, 30, 1), (5, 38, 9), (3, 24, 40), (2, 38, 9)]
    Bt, Tm, Lm = sum(s[0] for s in shapes), max(s[1] for s in shapes), max(s[2] for s in shapes)
    X = np.zeros((Bt, Tm, geom.feat), dtype=np.float32)
    X1 = np.zeros((Bt, Lm), dtype=np.int64)
    frames, canon = np.zeros(Bt, dtype=np.int32), np.zeros(Bt, dtype=np.int32)
    r = 0
    for k, (b, Tg, L) in enumerate(shapes):
        x, _, _, _ = synth.synth_batch(geom, B=b, T=Tg, L=L, seed=7 + 31 * k, ragged=True)
        X[r:r + b, :Tg] = x; X1[r:r + b, :L] = _ids(geom, b, L, start=11 * k); frames[r:r + b] = Tg // 2; canon[r:r + b] = L
        r += b
    args = (_cuda(X), _cuda(X1), _cuda(frames), _cuda(canon))
    want = old.forward_fused(*args, sync_errors=True).cpu().numpy()
    for _ in range(4):
        got = new.forward_fused(*args, sync_errors=True).cpu().numpy()
        for b in range(Bt):
            np.testing.assert_array_equal(got[:frames[b], b].view(np.int32), want[:frames[b], b].view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32x6", "f32"])
def test_text_table_follows_the_weights(precision):
    """A second state dict finalized on the same handle: the result is a fresh model's, so no row of the first set's table survived."""
    geom = synth.Geometry(**synth.REFERENCE)
    sd1, sd2 = synth.synth_state_dict(geom, seed=3), synth.synth_state_dict(geom, seed=4)
    B, L = 3, 40
    x, _, _, _ = synth.synth_batch(geom, B=B, T=T, L=L, seed=9, ragged=False)
    x1 = _ids(geom, B, L)
    m = _model(geom, sd1, precision)
    first = _run(m, x, x1)                       # (captures a graph that holds the first set's table)
    m.load_state_dict(sd2)
    second = _run(m, x, x1)
    _assert_same(second, _run(_model(geom, sd2, precision), x, x1))
    _assert_same(second, _run(_model(geom, sd2, precision, "gemm"), x, x1))
    assert not torch.equal(_bits(first[1]), _bits(second[1]))


@pytest.mark.gpu
def test_text_table_follows_the_precision():
    """mdd_set_precision from 2 to 0 and back on one handle: each result equals fresh models of that mode, table and per-call."""
    from ctc_attention_mispronunciation_amd import _lib
    geom, new6, old6 = _pair("ref", "f32x6")
    _, new0, old0 = _pair("ref", "f32")
    sd = synth.synth_state_dict(geom, seed=83)
    B, L = 3, 40
    x, _, _, _ = synth.synth_batch(geom, B=B, T=T, L=L, seed=2, ragged=False)
    x1 = _ids(geom, B, L)
    m = _model(geom, sd, "f32x6")
    want6, want0 = _run(old6, x, x1), _run(old0, x, x1)
    _assert_same(_run(new6, x, x1), want6)
    _assert_same(_run(new0, x, x1), want0)
    assert not torch.equal(_bits(want6[0]), _bits(want0[0]))     # the two arithmetics differ: a table of the wrong mode would show
    for mode, want in ((2, want6), (0, want0), (2, want6), (0, want0)):
        _lib.check(_lib.lib().mdd_set_precision(m.handle, mode))
        _assert_same(_run(m, x, x1), want)


@pytest.mark.gpu
def test_text_table_is_off_in_bf16x3():
    """Mode 1 keeps the per-call projection (the bf16x3 launcher picks its kernel by problem size: test_text_table_plan asserts the plan);
    the switch changes nothing there, and a handle that visits mode 1 comes back to the table."""
    from ctc_attention_mispronunciation_amd import _lib
    geom, new, old = _pair("ref", "bf16x3")
    assert new.precision == old.precision == "bf16x3"
    B, L = 3, 7
    x, _, _, _ = synth.synth_batch(geom, B=B, T=T, L=L, seed=6, ragged=False)
    x1 = _ids(geom, B, L)
    want = _run(old, x, x1)
    _assert_same(_run(new, x, x1), want)
    _, new6, old6 = _pair("ref", "f32x6")
    _lib.check(_lib.lib().mdd_set_precision(new.handle, 2))
    try:
        _assert_same(_run(new, x, x1), _run(old6, x, x1))
    finally:
        _lib.check(_lib.lib().mdd_set_precision(new.handle, 1))
    _assert_same(_run(new, x, x1), want)


_PLAN_DRIVER = r'''
#include <iostream>
#include <sstream>
#include <string>
#include "plan.h"
using namespace mdd;
// stdin, one case per line: hidden emb_dim mode B [SWITCH=value ...]  (other geometry: the reference's; every grid fits)
int main() {
    const char *env[] = {"MDD_PRECISION", "MDD_LSTM", "MDD_TEXT_PROJ", "MDD_SCORE_TILE"};
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        mdd_config c{243, 384, 4, 45, 32, 44, 512, 1e-5f};
        int mode, B;
        in >> c.hidden >> c.emb_dim >> mode >> B;
        for (const char *e : env) unsetenv(e);
        for (std::string kv; in >> kv;) setenv(kv.substr(0, kv.find('=')).c_str(), kv.substr(kv.find('=') + 1).c_str(), 1);
        const Switches sw = read_switches();
        const ForwardPlan p = plan_forward(c, mode, sw, DeviceFit{true, true, true}, B);
        std::cout << p.precision << ' ' << p.text_table << ' ' << sw.text_gemm << '\n';
    }
}
'''


def test_text_table_plan(tmp_path):
    """csrc/plan.h with the host compiler: the table is on in modes 0 and 2 (and where mode 2 falls back to 0), off in mode 1 and under
    MDD_TEXT_PROJ=gemm; any other value of the switch is its default."""
    drv = tmp_path / "plan_driver.cpp"
    drv.write_text(_PLAN_DRIVER)
    exe = str(tmp_path / "plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "ctc-attention-mispronunciation_amd", "csrc"),
                           str(drv), "-o", exe])
    cases = [("384 512 2 512", "2 1 0"), ("384 512 0 512", "0 1 0"), ("384 512 1 512", "1 0 0"),
             ("256 512 2 128", "2 1 0"), ("256 512 0 1", "0 1 0"), ("256 512 1 64", "1 0 0"),
             ("384 512 2 1025", "2 1 0"), ("384 512 2 512 MDD_LSTM=step", "2 1 0"),
             ("384 12 2 3", "0 1 0"), ("384 12 1 3", "0 1 0"),          # no planes of a 12-wide embedding: mode 0, and its table
             ("384 512 2 512 MDD_TEXT_PROJ=gemm", "2 0 1"), ("384 512 0 512 MDD_TEXT_PROJ=gemm", "0 0 1"),
             ("384 512 1 512 MDD_TEXT_PROJ=gemm", "1 0 1"), ("384 12 2 3 MDD_TEXT_PROJ=gemm", "0 0 1"),
             ("384 512 2 512 MDD_TEXT_PROJ=table", "2 1 0"), ("384 512 2 512 MDD_SCORE_TILE=128", "2 1 0")]
    r = subprocess.run([exe], input="\n".join(c for c, _ in cases) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = r.stdout.strip().split("\n")
    assert len(got) == len(cases)
    for (c, want), g in zip(cases, got):
        assert g == want, (c, g, want)
