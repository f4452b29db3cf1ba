"""The Python layer over the C ABI: ``_lib`` is the one place that turns objects into C arguments, ``hip_model.HipModel`` the one owner
of a decode handle, and the reference-shaped ``CTC_Model`` classes drive a HipModel -- so their results are HipModel's bit for bit, taps
are switched on once, bad canonical ids raise as before and a model follows its inputs to another device."""
import numpy as np
import pytest
import torch

from ctc_attention_mispronunciation_amd import _lib, synth


# ----------------------------------------------------------------------------- _lib (no GPU)
def test_ptr_of_none_numpy_and_tensor():
    a = np.arange(6, dtype=np.float32)
    t = torch.arange(6, dtype=torch.int64)
    assert _lib.ptr(None) is None
    assert _lib.ptr(a).value == a.ctypes.data
    assert _lib.ptr(t).value == t.data_ptr()
    assert _lib.ptr(t[2:]).value == t.data_ptr() + 16          # the object as given: no copy, no base address
    with pytest.raises(TypeError):
        _lib.ptr([1.0, 2.0])
    with pytest.raises(TypeError):
        _lib.ptr(a.ctypes.data)


def test_ptr_array_passes_none_as_null():
    t = torch.zeros(3)
    arr = _lib.ptr_array([t, None])
    assert len(arr) == 2 and arr[0] == t.data_ptr() and arr[1] is None
    assert len(_lib.ptr_array([])) == 0


def test_precisions_is_the_one_map():
    assert _lib.PRECISIONS == {"f32": 0, "bf16x3": 1, "f32x6": 2}


# ----------------------------------------------------------------------------- the classes (GPU)
B, T, L = 2, 32, 6                                             # smoke()'s shape
GEOM = synth.Geometry(**synth.REFERENCE_256)                   # (CTC_Model fixes the embedding at 44 x 512: the tiny geometry cannot load into it)
GEOM_CTC = synth.Geometry(ctc_only=True, **synth.TINY)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _drop_in(module, geom, sd):
    import torch.nn as nn
    model = module.CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=0.2)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return model.eval()


@pytest.fixture(scope="module")
def case():
    """One weight set and batch, the HipModel of them and its forward (left unchanged by the tests that share it)."""
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    sd = synth.synth_state_dict(GEOM, seed=1234)
    x, x1, _, _ = synth.synth_batch(GEOM, B=B, T=T, L=L, seed=5)
    x, x1 = torch.from_numpy(x), torch.from_numpy(x1)
    hip = HipModel(GEOM, sd)
    want = hip.forward(x.cuda(), x1.cuda(), sync_errors=True).clone()
    yield {"sd": sd, "x": x, "x1": x1, "hip": hip, "want": want}
    hip.close()


@pytest.mark.gpu
def test_forward_bits_are_hip_models(case):
    from ctc_attention_mispronunciation_amd.models import model_ctc
    model = _drop_in(model_ctc, GEOM, case["sd"])
    got = model(case["x"], case["x1"])
    assert not got.is_cuda and torch.equal(_bits(got), _bits(case["want"].cpu()))
    got = model(case["x"].cuda(), case["x1"].cuda())
    assert got.device == case["want"].device and torch.equal(_bits(got), _bits(case["want"]))
    assert model._hip.num_class == GEOM.num_class and model._hip.geom is None and model._hip.precision == case["hip"].precision


@pytest.mark.gpu
def test_ctc_only_forward_bits_are_hip_models():
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    from ctc_attention_mispronunciation_amd.models import cnn_rnn
    sd = synth.synth_state_dict(GEOM_CTC, seed=81)
    x = torch.from_numpy(synth.synth_batch(GEOM_CTC, B=3, T=8, L=2, seed=82)[0])
    hip = HipModel(GEOM_CTC, sd)
    want = hip.forward(x.cuda(), None, sync_errors=True)
    model = _drop_in(cnn_rnn, GEOM_CTC, sd)
    got = model(x, torch.ones((3, 2), dtype=torch.int64))       # x1 is accepted and ignored
    assert not got.is_cuda and torch.equal(_bits(got), _bits(want.cpu()))
    assert torch.equal(_bits(model(x.cuda(), None)), _bits(want))
    hip.close()


@pytest.mark.gpu
def test_candidates_bits_are_hip_models(case):
    from ctc_attention_mispronunciation_amd.models import model_ctc
    rng = np.random.Generator(np.random.PCG64(9))
    c0, c1 = (torch.from_numpy(rng.integers(1, GEOM.emb_rows, size=(B, n))) for n in (3, 6))
    ids = torch.zeros((2, B, 6), dtype=torch.int64)
    ids[0, :, :3], ids[1] = c0, c1
    canon = torch.tensor([3] * B + [6] * B, dtype=torch.int32)
    want = case["hip"].forward_candidates(case["x"].cuda(), ids.cuda(), canon=canon.cuda(), sync_errors=True)
    model = _drop_in(model_ctc, GEOM, case["sd"])
    for x, cands in ((case["x"], [c0, c1]), (case["x"].cuda(), [c0.cuda(), c1])):
        got = model.forward_candidates(x, cands)
        assert len(got) == 2
        for k in range(2):
            assert got[k].device == x.device and torch.equal(_bits(got[k].cpu()), _bits(want[k].cpu())), k


@pytest.mark.gpu
def test_taps_are_enabled_once(case, monkeypatch):
    from ctc_attention_mispronunciation_amd.models import model_ctc
    lib = _lib.lib()
    real, calls = lib.mdd_enable_taps, []

    def counted(handle, on):
        calls.append(on)
        return real(handle, on)

    monkeypatch.setattr(lib, "mdd_enable_taps", counted)
    model = _drop_in(model_ctc, GEOM, case["sd"])
    model.enable_taps(True)
    x, x1 = case["x"].cuda(), case["x1"].cuda()
    outs = [model(x, x1) for _ in range(3)]
    outs += model.forward_candidates(x, [x1])
    assert calls == [1]
    assert all(torch.equal(_bits(o), _bits(case["want"])) for o in outs[:3])
    rnn0 = model.tap("rnn0")
    assert rnn0.device == model._hip.device and rnn0.numel() == (T // 2) * B * 2 * GEOM.hidden
    out, visual = model(case["x"], case["x1"], visualize=True)
    assert calls == [1] and len(visual) == 4 and visual[0] is case["x"] and visual[3] is out
    assert visual[1].shape == (B, GEOM.channels, T // 2, GEOM.w2) and visual[2].shape == (T // 2, B, GEOM.rnn_in)
    assert torch.equal(_bits(out), _bits(case["want"].cpu()))
    model.enable_taps(False)
    model.enable_taps(False)
    assert calls == [1, 0]
    plain = _drop_in(model_ctc, GEOM, case["sd"])               # visualize alone switches the taps on, and leaves them on
    plain(x, x1, visualize=True)
    plain(x, x1, visualize=True)
    assert calls == [1, 0, 1] and plain.tap("conv1").numel() == (T // 2) * B * GEOM.rnn_in


@pytest.mark.gpu
def test_bad_ids_raise_index_error(case):
    from ctc_attention_mispronunciation_amd.models import model_ctc
    model = _drop_in(model_ctc, GEOM, case["sd"])
    bad = case["x1"].clone()
    bad[1, 2] = GEOM.emb_rows                                   # 44: one past the embedding's last row
    with pytest.raises(IndexError):
        model(case["x"], bad)
    with pytest.raises(IndexError):
        model.forward_candidates(case["x"], [case["x1"], bad])
    assert torch.equal(_bits(model(case["x"], case["x1"])), _bits(case["want"].cpu()))      # a good batch afterwards is served as ever
    model.strict_errors = False
    model(case["x"], bad)
    model.forward_candidates(case["x"], [case["x1"], bad])
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_model_follows_its_inputs_to_another_device(case):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    from ctc_attention_mispronunciation_amd.models import model_ctc
    model = _drop_in(model_ctc, GEOM, case["sd"])
    outs = []
    for index in (0, 1, 0):
        dev = torch.device("cuda", index)
        outs.append(model(case["x"].to(dev), case["x1"].to(dev)))
        assert outs[-1].device == dev and model._hip.device.index == index
    for out in outs:
        assert torch.equal(_bits(out.cpu()), _bits(case["want"].cpu()))
