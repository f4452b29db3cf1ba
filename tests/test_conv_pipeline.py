"""The default f32x6 conv front end against the row-at-a-time kernel (MDD_CONV=rowwise) at the smallest shapes at which its rotating
conv0 row slots, its per-lane bookkeeping hoisted out of the row loop and its split conv1 epilogue can go wrong: fill and drain of the
slots (T' = 1 .. 5), segment seams with a short last segment, the raw-frame path with the clamp to the last frame inside the last tile,
the fp32 tap on and off, repeated runs of one shape (a synchronisation slip shows as a mismatch in some repetition) and fused batches
of different padded lengths through a graph capture and replays.  Same products in the same order: every comparison is on the bits."""
import os

import numpy as np
import pytest
import torch

from ctc_attention_mispronunciation_amd import synth


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def models():
    """{taps: (default model, row-wise model)} of one set of weights; MDD_CONV is read when a model is created."""
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=4321)
    saved = os.environ.pop("MDD_CONV", None)
    made = {}
    try:
        for taps in (True, False):
            new = HipModel(geom, sd, precision="f32x6", taps=taps)
            os.environ["MDD_CONV"] = "rowwise"
            old = HipModel(geom, sd, precision="f32x6", taps=taps)
            del os.environ["MDD_CONV"]
            made[taps] = (new, old)
    finally:
        os.environ.pop("MDD_CONV", None)
        if saved is not None:
            os.environ["MDD_CONV"] = saved
    yield geom, made
    for new, old in made.values():
        new.close(); old.close()


def _check_forward(geom, pair, B, T, taps=True):
    new, old = pair
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=T, L=5, seed=17 * B + T, ragged=False)
    got = new.forward(_cuda(x), _cuda(x1), sync_errors=True)
    want = old.forward(_cuda(x), _cuda(x1), sync_errors=True)
    if taps:
        c_new, c_old = new.tap("conv1"), old.tap("conv1")
        assert c_new.numel() == (T // 2) * B * 1952
        assert torch.equal(_bits(c_new), _bits(c_old))
    assert torch.equal(_bits(got), _bits(want))


# T' = 1 .. 5: a first block alone, with one row and with two; a continuing block with one row and with two
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Tp", [1, 2, 3, 4, 5])
def test_conv_pipeline_fill_and_drain(B, Tp, models):
    geom, made = models
    _check_forward(geom, made[True], B, 2 * Tp)


# Segments per utterance = ceil(512 / B), rounded to whole blocks of two rows: (100, 32) -> T' = 16 in segments of 4; (200, 20) ->
# T' = 10 in segments 4, 4, 2 (a last segment of two rows); (100, 34) -> T' = 17 in segments 4, 4, 4, 4, 1 (of a single row)
@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(100, 32), (200, 20), (100, 34)])
def test_conv_pipeline_segment_seams(B, T, models):
    geom, made = models
    _check_forward(geom, made[True], B, T)


@pytest.mark.gpu
@pytest.mark.parametrize("T_raw", [5, 9, 253])
def test_conv_pipeline_raw_frames(T_raw, models):
    geom, made = models
    new, old = made[True]
    B = 2
    raw = torch.from_numpy(synth.synth_raw_features(B, T_raw, 81, seed=T_raw)).cuda()
    _, x1, _, _ = synth.synth_batch(geom, B=B, T=max(2, T_raw // 2 * 2), L=5, seed=3, ragged=False)
    got = new.forward_raw(raw, _cuda(x1), sync_errors=True)
    c_new = new.tap("conv1")
    want = old.forward_raw(raw, _cuda(x1), sync_errors=True)
    c_old = old.tap("conv1")
    assert c_new.numel() == c_old.numel() == got.shape[0] * B * 1952
    assert torch.equal(_bits(c_new), _bits(c_old))
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("taps", [True, False])
def test_conv_pipeline_taps_on_and_off(taps, models):
    geom, made = models
    _check_forward(geom, made[taps], 3, 14, taps=taps)


@pytest.mark.gpu
def test_conv_pipeline_race_screen(models):
    """One shape with several workgroups per utterance, eight runs on one model: every run must give the row-wise bits."""
    geom, made = models
    new, old = made[True]
    B, T = 64, 60
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=T, L=5, seed=99, ragged=False)
    xd, x1d = _cuda(x), _cuda(x1)
    want = old.forward(xd, x1d, sync_errors=True).clone()
    c_old = old.tap("conv1").clone()
    for rep in range(8):
        got = new.forward(xd, x1d, sync_errors=True)
        assert torch.equal(_bits(new.tap("conv1")), _bits(c_old)), rep
        assert torch.equal(_bits(got), _bits(want)), rep


@pytest.mark.gpu
def test_conv_pipeline_fused_batches_of_different_lengths(models):
    """T'_g = 1, 2, 3 and 6 in one forward_fused call: the capture, then two replays; each row compared up to its own length."""
    geom, made = models
    new, old = made[False]
    shapes = [(2, 2, 3), (3, 4, 2), (1, 6, 5), (2, 12, 4)]   # (rows, T_g, L_g)
    Bt, Tm, Lm = sum(s[0] for s in shapes), max(s[1] for s in shapes), max(s[2] for s in shapes)
    X = np.zeros((Bt, Tm, geom.feat), dtype=np.float32)
    X1 = np.zeros((Bt, Lm), dtype=np.int64)
    frames, canon = np.zeros(Bt, dtype=np.int32), np.zeros(Bt, dtype=np.int32)
    r = 0
    for k, (b, T, L) in enumerate(shapes):
        x, x1, _, _ = synth.synth_batch(geom, B=b, T=T, L=L, seed=11 + 7 * k, ragged=True)
        X[r:r + b, :T] = x; X1[r:r + b, :L] = x1; frames[r:r + b] = T // 2; canon[r:r + b] = L
        r += b
    args = (_cuda(X), _cuda(X1), _cuda(frames), _cuda(canon))
    want = old.forward_fused(*args, sync_errors=True).clone()
    for rep in range(3):
        got = new.forward_fused(*args, sync_errors=True)
        for b in range(Bt):
            assert torch.equal(_bits(got[:frames[b], b]), _bits(want[:frames[b], b])), (rep, b)
