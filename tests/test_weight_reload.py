"""Loading new weights into a live handle (mdd_finalize_weights again on the same model) gives exactly what a freshly built model
of those weights gives.  A finalize builds a whole new device weight set and swaps it in only when complete, so no kernel can
read a weight of the previous set; a finalize that fails leaves the handle unfinalized, and a later good load recovers it."""
import numpy as np
import pytest
import torch

from ctc_attention_mispronunciation_amd import synth

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _fresh(geom, sd, x, x1, precision):
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    m = HipModel(geom, sd, precision=precision)
    out = m.forward(x, x1, sync_errors=True).clone()
    m.close()
    return out


@pytest.mark.parametrize("precision", ["f32x6", "f32", "bf16x3"])
def test_refinalize_gives_fresh_model_bits(precision):
    """Reference geometry (H = 384) at B = 64, T = 100: in f32x6 every BiLSTM layer runs the x6 recurrence, which reads the
    three-plane W_hh.  Between the loads the device sees an unrelated allocation and a workspace growth, so a stale weight
    pointer would not happen to land on the new weights."""
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    geom = synth.Geometry(**synth.REFERENCE)
    sd_a, sd_b = synth.synth_state_dict(geom, seed=101), synth.synth_state_dict(geom, seed=202)
    x, x1, _, _ = synth.synth_batch(geom, B=64, T=100, L=20, seed=3)
    xg, x1g, _, _ = synth.synth_batch(geom, B=64, T=160, L=24, seed=4)
    x, x1, xg, x1g = _cuda(x), _cuda(x1), _cuda(xg), _cuda(x1g)
    m = HipModel(geom, sd_a, precision=precision)
    assert m.precision == precision
    out_a = m.forward(x, x1, sync_errors=True).clone()
    unrelated = torch.empty(48 << 20, dtype=torch.uint8, device="cuda")
    m.forward(xg, x1g, sync_errors=True)                       # grows the workspace
    m.load_state_dict(sd_b)
    out_b = m.forward(x, x1, sync_errors=True).clone()
    assert not _same_bits(out_a, out_b)                        # the two weight sets are told apart
    assert _same_bits(out_b, _fresh(geom, sd_b, x, x1, precision))
    m.load_state_dict(sd_a)
    assert _same_bits(m.forward(x, x1, sync_errors=True), out_a)
    del unrelated
    m.close()


def test_failed_finalize_leaves_unfinalized_handle():
    from ctc_attention_mispronunciation_amd import _lib
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    geom = synth.Geometry(**synth.REFERENCE)
    sd_a, sd_b = synth.synth_state_dict(geom, seed=101), synth.synth_state_dict(geom, seed=202)
    x, x1, _, _ = synth.synth_batch(geom, B=64, T=100, L=20, seed=3)
    x, x1 = _cuda(x), _cuda(x1)
    m = HipModel(geom, sd_a, precision="f32x6")
    m.forward(x, x1, sync_errors=True)
    bad = dict(sd_b)
    bad["score.weight"] = np.zeros((2 * geom.hidden + 1, 2 * geom.hidden), dtype=np.float32)
    with pytest.raises(_lib.MddError, match="score.weight"):
        m.load_state_dict(bad)
    with pytest.raises(_lib.MddError, match="finalize"):
        m.forward(x, x1, sync_errors=True)
    m.load_state_dict(sd_b)
    assert _same_bits(m.forward(x, x1, sync_errors=True), _fresh(geom, sd_b, x, x1, "f32x6"))
    m.close()


def test_ctc_model_mark_weights_changed_gives_fresh_model_bits():
    """The drop-in class at its default precision (f32x6): parameters edited in place, then mark_weights_changed()."""
    import torch.nn as nn
    from ctc_attention_mispronunciation_amd import _lib
    from ctc_attention_mispronunciation_amd.models.model_ctc import CTC_Model
    geom = synth.Geometry(**synth.REFERENCE)
    sd_a, sd_b = synth.synth_state_dict(geom, seed=101), synth.synth_state_dict(geom, seed=202)
    x, x1, _, _ = synth.synth_batch(geom, B=64, T=100, L=20, seed=3)
    x, x1 = _cuda(x), _cuda(x1)

    def make(sd):
        model = CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=0.2)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        return model.eval()

    model = make(sd_a)
    with torch.no_grad():
        out_a = model(x, x1).clone()
    assert _lib.lib().mdd_get_precision(model._hip.handle) == 2
    unrelated = torch.empty(48 << 20, dtype=torch.uint8, device="cuda")
    with torch.no_grad():
        for k, t in model.state_dict().items():
            if t.is_floating_point():
                t.copy_(torch.from_numpy(np.asarray(sd_b[k])))
    model.mark_weights_changed()
    with torch.no_grad():
        out_b = model(x, x1).clone()
        want = make(sd_b)(x, x1)
    assert not _same_bits(out_a, out_b)
    assert _same_bits(out_b, want)
    del unrelated
