"""Several canonical candidates per utterance on one acoustic pass: mdd_forward_candidates / HipModel.forward_candidates /
CTC_Model.forward_candidates / infer --pronunciations (include/mdd_hip.h, DESIGN.md "Candidates").

Shapes (weights synth.synth_state_dict, batches synth.synth_batch, candidate ids drawn per set from [2, emb_rows) by a seeded generator):

  a  synth.TINY      B 3  K 2  T 12  L 5   canon (5, 3)      scalar tail, step kernels
  b  H = 384         B 3  K 3  T 32  L 7   canon (7, 4, 1)   one 16-frame tile; L = 1
  c  H = 384         B 5  K 4  T 66  L 9   ragged frames     T' = 33: a partial frame tile; K B = 20: two 16-row LSTM tiles
  d  H = 384         B 2  K 2  T 16  L 65                    second 64-column score tile; strided softmax branch
  e  H = 256         B 48 K 3  T 16  L 6                     K B = 144 > 128: mode 2's plan leaves the f32x6 recurrence

Mode 1 (bf16x3) compares bit for bit at every one of them as well: launch_gemm_bf16x3 picks its kernel by problem size, but every kernel
it picks accumulates an output element in the same order (csrc/gemm_bf16x3.hip), so the allowance the float64 comparison would give a
shape is not taken.
"""
import contextlib
import ctypes as C
import functools
import io
import os
import shutil

import numpy as np
import pytest
import torch

from ctc_attention_mispronunciation_amd import _lib, synth
from tests.helpers import GOLD, jload, record_margin

pytestmark = pytest.mark.gpu

TOL = 1e-4     # the project's parity tolerance on the log-probs (README, tests/ctc_only_cases.TOL)
MODES = ["f32", "f32x6", "bf16x3"]
H256_2 = dict(feat=243, channels=32, hidden=256, layers=2, num_class=45)   # the refusals' geometry (tests/test_forward_call.py FUSED)
SHAPES = {
    "a": dict(geom=synth.TINY, B=3, K=2, T=12, L=5, canon=(5, 3), ragged=False),
    "b": dict(geom=synth.REFERENCE, B=3, K=3, T=32, L=7, canon=(7, 4, 1), ragged=False),
    "c": dict(geom=synth.REFERENCE, B=5, K=4, T=66, L=9, canon=None, ragged=True),
    "d": dict(geom=synth.REFERENCE, B=2, K=2, T=16, L=65, canon=None, ragged=False),
    "e": dict(geom=synth.REFERENCE_256, B=48, K=3, T=16, L=6, canon=None, ragged=False),
}


def _hip():
    from ctc_attention_mispronunciation_amd import hip_model
    return hip_model


@functools.lru_cache(maxsize=None)
def _weights(name):
    geom = synth.Geometry(**SHAPES[name]["geom"])
    return geom, synth.synth_state_dict(geom, seed=31)


@functools.lru_cache(maxsize=None)
def _model(name, precision):
    """One handle per (geometry, mode), shared by the tests (shapes b, c and d share the H = 384 one)."""
    gname = {"c": "b", "d": "b"}.get(name, name)
    if gname != name:
        return _model(gname, precision)
    geom, sd = _weights(name)
    m = _hip().HipModel(geom, sd, precision=precision)
    assert m.precision == ("f32" if name == "a" else precision)    # (TINY has no contraction length that is a multiple of 32: mode 0)
    return m


@functools.lru_cache(maxsize=None)
def _case(name):
    """Host inputs of one shape: x [B,T,F], x1 [K,B,L] (set k zero from its canon[k] on), frames [B] or None, canon [K] or None."""
    s = SHAPES[name]
    geom, _ = _weights(name)
    B, K, T, L = s["B"], s["K"], s["T"], s["L"]
    x, _, frac, _ = synth.synth_batch(geom, B=B, T=T, L=L, seed=40 + ord(name), ragged=s["ragged"])
    rng = np.random.Generator(np.random.PCG64(900 + ord(name)))
    x1 = rng.integers(2, geom.emb_rows, size=(K, B, L)).astype(np.int64)
    if s["canon"]:
        for k, n in enumerate(s["canon"]):
            x1[k, :, n:] = 0
    frames = (frac * np.float32(T // 2)).astype(np.int32) if s["ragged"] else None
    if frames is not None:
        assert frames.min() < T // 2 and frames[0] == T // 2
    return x, x1, frames, s["canon"]


def _dev(name, K=None):
    x, x1, frames, canon = _case(name)
    s = SHAPES[name]
    K = K or s["K"]
    xd = torch.from_numpy(x).cuda()
    x1d = torch.from_numpy(np.ascontiguousarray(x1[:K])).cuda()
    fd = None if frames is None else torch.from_numpy(frames).cuda()
    cd = None if canon is None else torch.tensor(canon[:K], dtype=torch.int32).repeat_interleave(s["B"]).cuda()
    return xd, x1d, fd, cd


def _candidates(m, name, K=None, repeats=3):
    """forward_candidates issued `repeats` times into fresh NaN-filled outputs; all results must agree (a replayed graph once started on
    stale buffers here).  Returns the first, [K,T',B,C] on the host."""
    xd, x1d, fd, cd = _dev(name, K)
    outs = []
    for _ in range(repeats):
        out = torch.full((x1d.shape[0], xd.shape[1] // 2, xd.shape[0], m.geom.num_class), float("nan"), dtype=torch.float32, device="cuda")
        r = m.forward_candidates(xd, x1d, frames=fd, canon=cd, out=out, sync_errors=True)
        assert r.data_ptr() == out.data_ptr()
        outs.append(r.cpu().numpy())
    for o in outs[1:]:
        np.testing.assert_array_equal(o, outs[0], err_msg="%s: repeated call" % name)
    return outs[0]


def _repeated_batch(m, name, K=None):
    """forward_fused on x repeated K times with the same frames / canon: [K,T',B,C] on the host."""
    xd, x1d, fd, cd = _dev(name, K)
    K, B, L = x1d.shape
    Tp = xd.shape[1] // 2
    frames = (torch.full((B,), Tp, dtype=torch.int32, device="cuda") if fd is None else fd).repeat(K)
    canon = torch.full((K * B,), L, dtype=torch.int32, device="cuda") if cd is None else cd
    out = m.forward_fused(xd.repeat(K, 1, 1), x1d.reshape(K * B, L), frames, canon, sync_errors=True)
    return out.cpu().numpy().reshape(Tp, K, B, -1).transpose(1, 0, 2, 3)


def _assert_rows_equal(name, got, want, what):
    frames = _case(name)[2]
    assert got.shape == want.shape and np.isfinite(want).all()
    for b in range(got.shape[2]):
        n = got.shape[1] if frames is None else int(frames[b])     # rows t >= frames[b] are undefined by the interface
        np.testing.assert_array_equal(got[:, :n, b], want[:, :n, b], err_msg="%s %s utterance %d" % (what, name, b))


# ------------------------------------------------------------------------------------------- 1. the repeated batch, bit for bit
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_candidates_equal_the_repeated_batch_bitwise(name, precision):
    """forward_candidates against forward_fused on x.repeat(K, 1, 1) with the same frames / canon: equal bit for bit on every defined row, in
    all three modes and at all five shapes (mode 1 included: see the module docstring); three calls give the same bits."""
    m = _model(name, precision)
    _assert_rows_equal(name, _candidates(m, name), _repeated_batch(m, name), "repeated batch")


@pytest.mark.parametrize("precision", ["f32x6", "bf16x3"])
def test_candidate_count_is_part_of_the_graph_key(precision):
    """K = 2, 3, 2 on one handle with the same x, x1, canon and output addresses and the same B, T, L, so that the count is all that tells
    the calls apart: each equals the repeated batch of its own K (the captured graph of one count must not serve another)."""
    m = _model("b", precision)
    xd, x1d, _, cd = _dev("b")
    B = xd.shape[0]
    out = torch.empty((x1d.shape[0], xd.shape[1] // 2, B, m.geom.num_class), dtype=torch.float32, device="cuda")
    for K in (2, 3, 2):
        out.fill_(float("nan"))
        r = m.forward_candidates(xd, x1d[:K], canon=cd[:K * B], out=out[:K], sync_errors=True)
        assert r.data_ptr() == out.data_ptr() and x1d[:K].is_contiguous() and x1d[:K].data_ptr() == x1d.data_ptr()
        _assert_rows_equal("b", r.cpu().numpy(), _repeated_batch(m, "b", K), "K=%d" % K)
        assert bool(torch.isnan(out[K:]).all())          # nothing written past the K sets asked for


# ------------------------------------------------------------------------------------------- 2. forward itself, bit for bit
def _forward_each(m, name, K=None):
    xd, x1d, _, _ = _dev(name, K)
    canon = SHAPES[name]["canon"]
    return np.stack([m.forward(xd, x1d[k][:, :(canon[k] if canon else x1d.shape[2])].contiguous(), sync_errors=True).cpu().numpy()
                     for k in range(x1d.shape[0])])


def _candidates_full_frames(m, name, K=None):
    xd, x1d, _, cd = _dev(name, K)
    return m.forward_candidates(xd, x1d, canon=cd, sync_errors=True).cpu().numpy()


@pytest.mark.parametrize("precision", ["f32", "f32x6"])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_candidates_equal_forward_bitwise(name, precision):
    """forward_candidates(...)[k] against forward(x, x1[k][:, :L_k]) where plan_forward gives B and K B rows the same kernels (TINY, H = 384),
    modes 0 and 2, every utterance at full length: bit for bit."""
    m = _model(name, precision)
    np.testing.assert_array_equal(_candidates_full_frames(m, name), _forward_each(m, name))


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_one_candidate_set_is_forward_bitwise(name, precision):
    """K = 1 runs under forward's own plan: equal to forward at all five shapes, in every mode."""
    m = _model(name, precision)
    np.testing.assert_array_equal(_candidates_full_frames(m, name, 1), _forward_each(m, name, 1))


# ------------------------------------------------------------------------------------------- 3. float64
@functools.lru_cache(maxsize=None)
def _float64(name):
    """oracle.ref_port.forward in float64 of every candidate, [K,T',B,C].  With ragged frames an utterance is evaluated as the batch it
    stands for: its own T_g = 2 frames[b] frames (nothing of an eval forward crosses utterances, so one utterance is such a batch)."""
    from oracle import ref_port
    x, x1, frames, canon = _case(name)
    _, sd = _weights(name)
    K, B, L = x1.shape
    ref = np.full((K, x.shape[1] // 2, B, SHAPES[name]["geom"]["num_class"]), np.nan)
    for k in range(K):
        ids = x1[k][:, :(canon[k] if canon else L)]
        if frames is None:
            ref[k] = ref_port.forward(sd, x, ids, dtype=torch.float64).numpy()
        else:
            for b in range(B):
                n = int(frames[b])
                ref[k, :n, b] = ref_port.forward(sd, x[b:b + 1, :2 * n], ids[b:b + 1], dtype=torch.float64).numpy()[:, 0]
    return ref


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_candidates_against_float64(name, precision):
    """Every candidate of every shape within the parity tolerance 1e-4 of the reference graph in float64, in all three modes (at shape e,
    mode 2, this also bounds the distance between the plan of K B = 144 rows and forward's own plan of B = 48).  The existing margins at
    these lengths and weights are <= 1.2e-5 (profiles/candidates_margins.json holds these)."""
    got, ref = _candidates(_model(name, precision), name, repeats=1), _float64(name)
    frames = _case(name)[2]
    worst = 0.0
    for b in range(got.shape[2]):
        n = got.shape[1] if frames is None else int(frames[b])
        worst = max(worst, float(np.abs(got[:, :n, b] - ref[:, :n, b]).max()))
    print("candidates %s %s: max |logp - float64| = %.3e" % (name, precision, worst))
    record_margin("candidates_%s_%s_vs_float64" % (name, precision), worst, TOL)
    assert worst <= TOL


# ------------------------------------------------------------------------------------------- 4. drop-in
def _torch_model(geom, sd, ctc_only=False):
    import torch.nn as nn
    if ctc_only:
        from ctc_attention_mispronunciation_amd.models.cnn_rnn import CTC_Model
    else:
        from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    model = CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=0.2)
    if sd is not None:
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return model.eval()


def test_drop_in_forward_candidates():
    """CTC_Model.forward_candidates(x_host, [c0, c1, c2]) with lengths 6, 4, 6 at H = 384: three host tensors, each equal bit for bit to
    model(x_host, c_k); a model in train mode and the CTC-only class refuse."""
    geom, sd = _weights("b")
    model = _torch_model(geom, sd)
    x, _, _, _ = synth.synth_batch(geom, B=3, T=16, L=6, seed=77, ragged=False)
    rng = np.random.Generator(np.random.PCG64(78))
    cands = [torch.from_numpy(rng.integers(2, geom.emb_rows, size=(3, n)).astype(np.int64)) for n in (6, 4, 6)]
    xh = torch.from_numpy(x)
    got = model.forward_candidates(xh, cands)
    assert isinstance(got, list) and len(got) == 3
    for k, c in enumerate(cands):
        want = model(xh, c)
        assert got[k].device.type == "cpu" and got[k].shape == want.shape == (8, 3, geom.num_class)
        assert torch.equal(got[k], want), k
    on_dev = model.forward_candidates(xh.cuda(), [c.cuda() for c in cands])
    assert all(o.is_cuda and torch.equal(o.cpu(), g) for o, g in zip(on_dev, got))
    model.train()
    with pytest.raises(NotImplementedError, match="eval"):
        model.forward_candidates(xh, cands)
    baseline = _torch_model(synth.Geometry(ctc_only=True, **synth.REFERENCE), None, ctc_only=True)
    with pytest.raises(NotImplementedError, match="no canonical side"):
        baseline.forward_candidates(xh, cands)


# ------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_name_the_argument_and_leave_nothing_behind():
    """K = 0, x1_dev NULL, a CTC-only handle, an odd T, L one past max_canonical_len: -1 (MDD_ERR_ARG) with the argument named in
    mdd_last_error(), the sentinel-filled output untouched; an id equal to emb_rows in candidate set 1 is reported by mdd_sync; after each
    of them the handle still gives its first result."""
    lib = _lib.lib()
    geom = synth.Geometry(**H256_2)
    sd = synth.synth_state_dict(geom, seed=21)
    B, K, T, L = 3, 2, 16, 4
    x, _, _, _ = synth.synth_batch(geom, B=B, T=T, L=L, seed=5, ragged=False)
    xd = torch.from_numpy(x).cuda()
    rng = np.random.Generator(np.random.PCG64(6))
    x1 = torch.from_numpy(rng.integers(2, geom.emb_rows, size=(K, B, L)).astype(np.int64)).cuda()
    m = _hip().HipModel(geom, sd)
    want = m.forward_candidates(xd, x1, sync_errors=True).cpu().numpy()
    ctc_geom = synth.Geometry(ctc_only=True, **H256_2)
    ctc = _hip().HipModel(ctc_geom, synth.synth_state_dict(ctc_geom, seed=21))
    Lmax = 2364 - 2 * geom.hidden      # csrc/plan.h max_canonical_len with the matrix-core tail
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    st = _lib.current_stream_ptr()
    out = torch.empty((K, T // 2, B, geom.num_class), dtype=torch.float32, device="cuda")
    refused = [("K=0", lambda: lib.mdd_forward_candidates(m.handle, p(xd), B, T, p(x1), 0, L, None, None, p(out), st)),
               ("x1_dev", lambda: lib.mdd_forward_candidates(m.handle, p(xd), B, T, None, K, L, None, None, p(out), st)),
               ("CTC-only", lambda: lib.mdd_forward_candidates(ctc.handle, p(xd), B, T, p(x1), K, L, None, None, p(out), st)),
               ("T=15", lambda: lib.mdd_forward_candidates(m.handle, p(xd), B, T - 1, p(x1), K, L, None, None, p(out), st)),
               ("L=%d" % (Lmax + 1), lambda: lib.mdd_forward_candidates(m.handle, p(xd), B, T, p(x1), K, Lmax + 1, None, None, p(out), st))]
    for named, call in refused:
        out.fill_(-7.0)
        assert call() == -1, named                                  # MDD_ERR_ARG
        assert named in lib.mdd_last_error().decode(), (named, lib.mdd_last_error().decode())
        assert lib.mdd_sync(m.handle, st) == 0
        assert bool((out == -7.0).all()), named
        np.testing.assert_array_equal(m.forward_candidates(xd, x1, sync_errors=True).cpu().numpy(), want, err_msg=named)
    # L = max_canonical_len itself is not refused by this check (the same bound as mdd_forward); not run: its workspace is not the point here
    bad = x1.clone()
    bad[1, 2, 1] = geom.emb_rows
    assert lib.mdd_forward_candidates(m.handle, p(xd), B, T, p(bad), K, L, None, None, p(out), st) == 0
    assert lib.mdd_sync(m.handle, st) == -1 and "index out of range" in lib.mdd_last_error().decode()
    np.testing.assert_array_equal(m.forward_candidates(xd, x1, sync_errors=True).cpu().numpy(), want)
    with pytest.raises(IndexError):
        m.forward_candidates(xd, bad, sync_errors=True)
    m.close()
    ctc.close()


# ------------------------------------------------------------------------------------------- 6. infer --pronunciations
VOCAB_DIR = os.path.join(GOLD, "vocabulary_single")
TWO = {"accept", "content", "thorough", "toronto"}     # the words of vocabulary_single with a (2) entry in cmudict_subset.dict


def _volatile(line, tmp):
    """Lines of the program's output that differ from run to run: those that print a path of the run's own folder, and the timings."""
    return tmp in line or line.startswith(("RTF: ", "init model time: ", "process time: "))


def _run_infer(tmp_path, extra):
    from ctc_attention_mispronunciation_amd import infer as infer_cli
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = infer_cli.main(["--conf", str(tmp_path / "conf.yaml"), "--wav_transcript_path", str(tmp_path / "words"),
                             "--cmvn", os.path.join(GOLD, "global_fbank_cmvn.txt"), "--cmudict", os.path.join(GOLD, "cmudict_subset.dict")] + extra)
    assert rc == 0
    return buf.getvalue()


def _blocks(stdout):
    """utterance id -> the lines of its printed block, without the closing empty line (the first empty line behind 'score  :'; the
    translation line in the middle of a block is empty too)."""
    blocks, cur, scored = {}, None, False
    for line in stdout.split("\n"):
        if line.startswith("id     : "):
            cur, scored = blocks.setdefault(line[len("id     : "):], []), False
        if cur is not None:
            scored = scored or line.startswith("score  : ")
            if line == "" and scored:
                cur = None
            else:
                cur.append(line)
    return blocks


def test_infer_pronunciations_end_to_end(tmp_path, monkeypatch):
    """infer over tests/golden/vocabulary_single with cmudict_subset.dict and the seed-11 H = 384 checkpoint (the set-up of
    tests/test_infer_batch.py::test_cli_end_to_end), the program's main() run in this process.
    Without --pronunciations the output equals the recorded output of the same command on the commit before the flag existed
    (tests/golden/infer_single_stdout_before_pronunciations.txt; lines that print the run's folder and the three timing lines left out).
    With it: the 14 words with one pronunciation print the block they print without it plus a 'pron' line; for accept, content, thorough
    and toronto the choice is recomputed here -- the batch WavBatchLoader forms, two plain forwards on the two candidate sets,
    ctc_variants' base per candidate, the argmax with ties to the first -- and the printed block must be that candidate's diagnosis."""
    import torch.nn as nn  # noqa: F401
    from ctc_attention_mispronunciation_amd import infer as infer_cli
    from ctc_attention_mispronunciation_amd.dict.phonetic_dict import Phonetic
    from ctc_attention_mispronunciation_amd.hip_model import ctc_variants
    from ctc_attention_mispronunciation_amd.infer_core import diagnose
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    from ctc_attention_mispronunciation_amd.utils.ctcDecoder import BeamDecoder
    from ctc_attention_mispronunciation_amd.utils.data_loader import Vocab, WavBatchLoader, frames_from_fraction
    monkeypatch.delenv("MDD_PRECISION", raising=False)
    shutil.copytree(VOCAB_DIR, str(tmp_path / "words"))
    i2c = synth.phone_table_41()
    (tmp_path / "units").write_text("".join(i2c[i] + "\n" for i in range(2, len(i2c))))
    geom = synth.Geometry(**synth.REFERENCE)
    model = _torch_model(geom, synth.synth_state_dict(geom, seed=11))
    os.makedirs(str(tmp_path / "ckpt" / "exp"))
    torch.save(CTC_Model.save_package(model), str(tmp_path / "ckpt" / "exp" / "ctc_best_model.pkl"))
    arpa = os.path.join(GOLD, "lm_synth45.arpa")
    (tmp_path / "conf.yaml").write_text("exp_name: 'exp'\ncheckpoint_dir: '%s'\nvocab_file: '%s'\nleft_ctx: 0\nright_ctx: 2\nn_skip_frame: 2\n"
                                        "n_downsample: 2\nbatch_size: 64\ndecode_type: 'Beam'\nbeam_width: 10\nlm_path: '%s'\nlm_alpha: 0\n"
                                        % (tmp_path / "ckpt", tmp_path / "units", arpa))
    plain = _run_infer(tmp_path, [])
    kept = "".join(line + "\n" for line in plain.split("\n")[:-1] if not _volatile(line, str(tmp_path)))
    with open(os.path.join(GOLD, "infer_single_stdout_before_pronunciations.txt")) as f:
        assert kept == f.read()
    assert jload("g13_infer.json")["cases"][0]["batch_size"] == 64 and jload("g13_infer.json")["cases"][0]["stdout"] in plain

    flagged = _run_infer(tmp_path, ["--pronunciations"])
    before, after = _blocks(plain), _blocks(flagged)
    assert sorted(before) == sorted(after) and len(after) == 18

    # the test's own evaluation of the two candidate sets
    with contextlib.redirect_stdout(io.StringIO()):
        vocab = Vocab(str(tmp_path / "units"))
        items, word_dict, transcripts, _ = infer_cli.collect(str(tmp_path / "words"), Phonetic(os.path.join(GOLD, "cmudict_subset.dict")), True)
    words = {u: transcripts[u].strip().lower() for u in transcripts}
    assert TWO <= set(words.values())
    cmvn = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt")))
    batches = list(WavBatchLoader(items, vocab, 64, cmvn=cmvn, pronunciations=True))
    assert len(batches) == 1
    inputs, input_sizes, _, _, trans, trans_sizes, utts, cand = batches[0]
    assert len(cand["sets"]) == 2 and torch.equal(cand["sets"][0][0], trans) and torch.equal(cand["sets"][0][1], trans_sizes)
    beam = BeamDecoder(i2c, beam_width=10, blank_index=0, space_idx=-1, lm_path=arpa, lm_alpha=0.0)
    per_set = []
    for ids, sizes in cand["sets"]:
        probs = model(inputs, ids.cuda())
        lens = frames_from_fraction(input_sizes, probs.size(0)).numpy().tolist()
        base = ctc_variants(probs, lens, ids.to(torch.int32), sizes.to(torch.int32), 0, want_ins=False).base.cpu().tolist()
        per_set.append((beam.decode(probs, lens), ids.numpy(), sizes.numpy(), base))
    seen_two, picked = set(), {}
    for x, u in enumerate(utts):
        n = cand["counts"][x]
        assert n == (2 if words[u] in TWO else len(Phonetic(os.path.join(GOLD, "cmudict_subset.dict")).cmu_dict_all(words[u])))
        phones = [" ".join(i2c[i] for i in per_set[k][1][x][:per_set[k][2][x]]) for k in range(n)]
        ll = [per_set[k][3][x] for k in range(n)]
        chosen = max(range(n), key=lambda k: (ll[k], -k))              # the argmax, ties to the earlier entry
        pron = "pron   : " + " | ".join("%s%s [%.4f]" % ("*" if k == chosen else "", phones[k], ll[k]) for k in range(n))
        assert after[u][-1] == pron, (u, after[u][-1], pron)
        if n == 1:
            assert after[u][:-1] == before[u], u                       # today's block plus the pron line
            continue
        seen_two.add(words[u])
        assert len(set(phones)) == n and all(np.isfinite(ll))
        d = diagnose(per_set[chosen][0][x], phones[chosen], beam)
        tmp1, tmp2, tmp3 = d["printed"]
        want = ["id     : " + u, u + ": " + transcripts[u], word_dict[u]["cmu_all"][chosen], "", tmp2, tmp3, tmp1,
                "ins err: " + " ".join(d["insertions"]), "sub err: " + " ".join(d["substitutions"]), "del err: " + " ".join(d["deletions"]),
                "Comp.  : " + str(d["correct"]) + "/" + str(d["correct"] + d["del_sub"]), "score  : " + str(d["score"]), pron]
        assert after[u] == want, (u, after[u], want)
        picked[u] = (n, chosen, phones[chosen])
    assert TWO <= seen_two

    # --timestamps and --posteriors: the lines they add are the chosen candidate's too, in front of the pron line
    both = ["--timestamps", "--posteriors"]
    before_t, after_t = _blocks(_run_infer(tmp_path, both)), _blocks(_run_infer(tmp_path, both + ["--pronunciations"]))
    for u in utts:
        n, chosen, phones = picked.get(u, (1, 0, None))
        assert after_t[u][-1] == after[u][-1], u                       # the same choice and likelihoods
        assert after_t[u][:12] == after[u][:12], u
        assert [line[:9] for line in after_t[u][12:]] == ["time   : ", "gop    : ", "post   : ", "pron   : "], u
        if chosen == 0:                                                # the first entry's block is the one printed without --pronunciations
            assert after_t[u][:-1] == before_t[u], u
        else:                                                          # gop and post walk the chosen pronunciation's phonemes
            for line in after_t[u][13:15]:
                assert [tok.split("[")[0] for tok in line[9:].split("] ")] == phones.split(), (u, line)
