"""The attention scores on the 128 x 64 block tile of gemm_nt_f32_kernel (waves 4 x 1, taken where N = L <= 64) against the 128 x 128 tile
(MDD_SCORE_TILE=128): same MFMA, same K-tile, same flush cadence, so every score is the same fmaf chain and the "score" tap and the
log-probs must agree bit for bit.  L on both sides of the MFMA tile (32) and of the narrow tile (64); at L = 65 and 130 the launcher's
rule (N <= 64) leaves both models on the wide tile.  T' below one MFMA tile, one wave's rows (32 in the narrow form, 64 in the wide one),
one block tile (128) and just past it."""
import os

import numpy as np
import pytest
import torch

from ctc_attention_mispronunciation_amd import synth

B = 3
_PAIRS = {}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pair(geom_kw):
    """(64-column model, 128-column model) of one geometry and weight set; MDD_SCORE_TILE is read when a model is created."""
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    key = geom_kw["hidden"]
    if key not in _PAIRS:
        geom = synth.Geometry(**geom_kw)
        sd = synth.synth_state_dict(geom, seed=29)
        saved = os.environ.pop("MDD_SCORE_TILE", None)
        try:
            new = HipModel(geom, sd)
            os.environ["MDD_SCORE_TILE"] = "128"
            old = HipModel(geom, sd)
        finally:
            os.environ.pop("MDD_SCORE_TILE", None)
            if saved is not None:
                os.environ["MDD_SCORE_TILE"] = saved
        _PAIRS[key] = (geom, new, old)
    return _PAIRS[key]


def _run(m, x, x1):
    out = m.forward(_cuda(x), _cuda(x1), sync_errors=True).clone()
    return out, m.tap("score").clone()


@pytest.mark.gpu
@pytest.mark.parametrize("Tp", [1, 16, 125, 129])
@pytest.mark.parametrize("L", [1, 31, 32, 33, 40, 63, 64, 65, 130])
def test_score_tile_64_equals_128(L, Tp):
    geom, new, old = _pair(synth.REFERENCE)
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=2 * Tp, L=L, seed=L + Tp, ragged=True)
    (got, g_s), (want, w_s) = _run(new, x, x1), _run(old, x, x1)
    assert g_s.numel() == w_s.numel() == B * Tp * L
    assert torch.equal(_bits(g_s), _bits(w_s))
    assert torch.isfinite(g_s).all() and float(g_s.abs().max()) > 0.0
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.gpu
def test_score_tile_64_equals_128_h256():
    geom, new, old = _pair(synth.REFERENCE_256)
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=258, L=33, seed=4, ragged=True)
    (got, g_s), (want, w_s) = _run(new, x, x1), _run(old, x, x1)
    assert torch.equal(_bits(g_s), _bits(w_s))
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.gpu
def test_score_tile_fused_ragged_lengths():
    """Batches of different canonical lengths L_g and frame counts in one fused launch sequence: the scores are computed over the common
    L = 40 on both tiles (the tail picks each row's own l < L_g), through the capture and a replay."""
    geom, new, old = _pair(synth.REFERENCE)
    shapes = [(2, 60, 1), (3, 34, 33), (1, 258, 40), (2, 120, 7)]
    Bt, Tm, Lm = sum(s[0] for s in shapes), max(s[1] for s in shapes), max(s[2] for s in shapes)
    X = np.zeros((Bt, Tm, geom.feat), dtype=np.float32)
    X1 = np.zeros((Bt, Lm), dtype=np.int64)
    frames, canon = np.zeros(Bt, dtype=np.int32), np.zeros(Bt, dtype=np.int32)
    r = 0
    for k, (b, T, L) in enumerate(shapes):
        x, x1, _, _ = synth.synth_batch(geom, B=b, T=T, L=L, seed=3 + 17 * k, ragged=True)
        X[r:r + b, :T] = x; X1[r:r + b, :L] = x1; frames[r:r + b] = T // 2; canon[r:r + b] = L
        r += b
    args = (_cuda(X), _cuda(X1), _cuda(frames), _cuda(canon))
    want = old.forward_fused(*args, sync_errors=True).cpu().numpy()
    w_s = old.tap("score").clone()
    for _ in range(2):
        got = new.forward_fused(*args, sync_errors=True).cpu().numpy()
        assert torch.equal(_bits(new.tap("score")), _bits(w_s))
        for b in range(Bt):
            np.testing.assert_array_equal(got[:frames[b], b].view(np.int32), want[:frames[b], b].view(np.int32))
