"""The multi-row fused conv front end (conv_fused_kernel<3, R>, the f32x6 default) against the row-at-a-time kernel it replaced
(MDD_CONV=rowwise): the same products in the same order, so the conv1 tap and the log-probs must agree bit for bit -- batch sizes
1 .. 512, T' below R and not a multiple of R, several segments per utterance, the raw-frame path (stack/skip folded into the tile
load) with odd lengths, and fused batches of different padded lengths through graph replays."""
import numpy as np
import pytest
import torch

from ctc_attention_mispronunciation_amd import synth


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pair(monkeypatch, geom, sd, taps=False):
    """(multi-row model, row-wise model) of the same weights; MDD_CONV is read when a model is created."""
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    monkeypatch.delenv("MDD_CONV", raising=False)
    new = HipModel(geom, sd, precision="f32x6", taps=taps)
    monkeypatch.setenv("MDD_CONV", "rowwise")
    old = HipModel(geom, sd, precision="f32x6", taps=taps)
    monkeypatch.delenv("MDD_CONV")
    return new, old


# T' = T // 2: 1 (below R), 19 (odd; one-row segments rounded up to two), 250, 61, 101 (short odd last segment), 250 at B = 512
@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(1, 2), (1, 38), (2, 500), (3, 122), (64, 202), (64, 500), (512, 500)])
def test_conv_multirow_equals_rowwise(B, T, monkeypatch):
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=77)
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=T, L=7, seed=B + T, ragged=False)
    new, old = _pair(monkeypatch, geom, sd, taps=True)
    got = new.forward(_cuda(x), _cuda(x1), sync_errors=True)
    c_new = new.tap("conv1").clone()
    want = old.forward(_cuda(x), _cuda(x1), sync_errors=True)
    c_old = old.tap("conv1").clone()
    assert c_new.numel() == (T // 2) * B * 1952
    assert torch.equal(c_new.view(torch.int32), c_old.view(torch.int32))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("B,T_raw", [(3, 997), (3, 7), (1, 251), (64, 1001)])
def test_conv_multirow_raw_equals_rowwise(B, T_raw, monkeypatch):
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=5)
    raw = torch.from_numpy(synth.synth_raw_features(B, T_raw, 81, seed=T_raw)).cuda()
    _, x1, _, _ = synth.synth_batch(geom, B=B, T=max(2, T_raw // 2 * 2), L=5, seed=1, ragged=False)
    new, old = _pair(monkeypatch, geom, sd)
    got = new.forward_raw(raw, _cuda(x1), sync_errors=True)
    want = old.forward_raw(raw, _cuda(x1), sync_errors=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.gpu
def test_conv_multirow_fused_batches_equal_rowwise(monkeypatch):
    """Batches of different padded lengths in one fused launch sequence, then three replays of the captured graph."""
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=1234)
    shapes = [(5, 120, 9), (3, 64, 4), (7, 100, 12), (2, 120, 12), (4, 30, 1), (1, 2, 2)]
    Bt, Tm, Lm = sum(s[0] for s in shapes), max(s[1] for s in shapes), max(s[2] for s in shapes)
    X = np.zeros((Bt, Tm, geom.feat), dtype=np.float32)
    X1 = np.zeros((Bt, Lm), dtype=np.int64)
    frames, canon = np.zeros(Bt, dtype=np.int32), np.zeros(Bt, dtype=np.int32)
    r = 0
    for k, (b, T, L) in enumerate(shapes):
        x, x1, _, _ = synth.synth_batch(geom, B=b, T=T, L=L, seed=7 + 31 * k, ragged=True)
        X[r:r + b, :T] = x; X1[r:r + b, :L] = x1; frames[r:r + b] = T // 2; canon[r:r + b] = L
        r += b
    new, old = _pair(monkeypatch, geom, sd)
    args = (_cuda(X), _cuda(X1), _cuda(frames), _cuda(canon))
    want = old.forward_fused(*args, sync_errors=True).cpu().numpy()
    for _ in range(4):   # the first call captures the graph, the next three replay it
        got = new.forward_fused(*args, sync_errors=True).cpu().numpy()
        for b in range(Bt):
            np.testing.assert_array_equal(got[:frames[b], b].view(np.int32), want[:frames[b], b].view(np.int32))

