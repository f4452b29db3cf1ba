"""The training handle's contract around its saved forward (include/mdd_hip.h): a forward serves ONE backward, a backward follows the
kernels its own forward chose, a refused forward leaves nothing to run a backward on, and the tensor table keeps its order.  All through
TrainHandle on raw device tensors (no autograd), at the smallest shapes that reach the paths."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.helpers import jload
from tests.test_gpu_parity import _train_model, _cuda
from ctc_attention_mispronunciation_amd import synth

pytestmark = pytest.mark.gpu

MDD_ERR_ARG = -1
SENTINEL = -7.5


def _L():
    from ctc_attention_mispronunciation_amd import _lib
    return _lib.lib()


def _config(geom):
    from ctc_attention_mispronunciation_amd import _lib
    return _lib.MddConfig(feat=geom.feat, hidden=geom.hidden, layers=geom.layers, num_class=geom.num_class, channels=geom.channels,
                          emb_rows=geom.emb_rows, emb_dim=geom.emb_dim, bn_eps=1e-5)


@functools.lru_cache(maxsize=None)
def _case(H, B, T, L):
    geom = synth.Geometry(**dict(synth.REFERENCE, hidden=H))
    sd, x, x1, masks, _, _, _ = synth.train_case(geom, 77, B, T, L, 1)
    rs = np.random.Generator(np.random.PCG64(3))
    dlogp = (rs.standard_normal((T // 2, B, geom.num_class)) / B).astype(np.float32)
    return geom, sd, x, x1, masks, dlogp


class _Step(object):
    """A handle with the case's tensors on the device"""

    def __init__(self, H, B, T, L, mode=0):
        from ctc_attention_mispronunciation_amd.train import TrainHandle
        self.geom, sd, x, x1, masks, dlogp = _case(H, B, T, L)
        self.h = TrainHandle(_config(self.geom), 0)
        assert _L().mdd_train_set_precision(self.h.handle, mode) == 0
        self.tensors = [_cuda(np.asarray(sd[k]).reshape(-1)) for k in self.h.keys]
        self.x, self.x1, self.masks, self.dlogp = _cuda(x), _cuda(x1), [_cuda(m) for m in masks], _cuda(dlogp)

    def forward(self, x=None, masks=None):
        return self.h.forward(self.tensors, self.x if x is None else x, self.x1, self.masks if masks is None else masks, 0, 0.2)

    def backward(self):
        """(status, message, gradient buffers prefilled with the sentinel)"""
        h = self.h
        grads = [None if b else torch.full((n,), SENTINEL, device="cuda") for n, b in zip(h.numel, h.is_buffer)]
        from ctc_attention_mispronunciation_amd import _lib
        rc = _L().mdd_train_backward(h.handle, h._ptr_array(self.tensors), C.c_void_p(self.dlogp.data_ptr()), h._ptr_array(grads), _lib.current_stream_ptr())
        msg = _L().mdd_last_error().decode() if rc else ""
        torch.cuda.synchronize()
        return rc, msg, {k: g for k, g in zip(h.keys, grads) if g is not None}


def _refused(rc, msg, grads):
    assert rc == MDD_ERR_ARG and "forward first" in msg, (rc, msg)
    for k, g in grads.items():
        assert bool((g == SENTINEL).all()), k


def test_backward_runs_once_per_forward():
    """The backward overwrites activations the forward saved (the classifier's input with dX), so a second backward on the same forward
    used to return a wrong fc.1.weight gradient: it is refused with MDD_ERR_ARG ("forward first") and writes nothing, as is a backward
    on a handle that never ran a forward; after a new forward the backward gives the first result again, bit for bit."""
    s = _Step(256, 2, 4, 1)
    _refused(*s.backward())                                   # fresh handle
    s.forward()
    rc, msg, first = s.backward()
    assert rc == 0, msg
    assert all(not bool((g == SENTINEL).any()) for g in first.values())
    _refused(*s.backward())                                   # second backward on one forward
    s.forward()
    rc, msg, again = s.backward()
    assert rc == 0, msg
    for k in first:
        assert torch.equal(first[k], again[k]), k


def test_backward_follows_the_mode_of_its_forward():
    """mdd_train_set_precision between a forward and its backward: the backward still takes the kernels of its forward's mode.  H = 256,
    B = 8, T = 32, L = 4: 128 rows, dW_ih and dX of layers 1-3 are 2048 x 512 x 128 = 2^27 multiply-adds, the smallest mode 2 takes; the
    two modes must differ in rnns.1's weight_ih gradient there, or the comparison would say nothing."""
    shape = (256, 8, 32, 4)
    stayed = {}
    for mode in (0, 2):
        s = _Step(*shape, mode=mode)
        s.forward()
        rc, msg, stayed[mode] = s.backward()
        assert rc == 0, msg
    k = "rnns.1.rnn.weight_ih_l0"
    assert not torch.equal(stayed[0][k], stayed[2][k])
    for mode, other in ((2, 0), (0, 2)):
        s = _Step(*shape, mode=mode)
        s.forward()
        assert _L().mdd_train_set_precision(s.h.handle, other) == 0
        rc, msg, got = s.backward()
        assert rc == 0, msg
        for key in got:
            assert torch.equal(got[key], stayed[mode][key]), (mode, other, key)


def test_refused_forward_leaves_no_saved_forward():
    """A forward that is refused (odd T; one dropout mask missing) after a good one: the good one's activations are no longer trusted,
    a backward is refused and writes nothing."""
    from ctc_attention_mispronunciation_amd._lib import MddError
    s = _Step(256, 2, 4, 1)
    for bad in (dict(x=s.x[:, :3].contiguous()), dict(masks=s.masks[:-1] + [None])):
        s.forward()
        with pytest.raises(MddError):
            s.forward(**bad)
        _refused(*s.backward())
    s.forward()
    assert s.backward()[0] == 0


@pytest.mark.parametrize("name,geom", [("reference_H384", synth.REFERENCE), ("tiny", synth.TINY)])
def test_tensor_table_order(name, geom):
    """mdd_train_tensor_info lists (key, numel, is_buffer) exactly as the library did before the table was resolved into indices at create
    (tests/golden/train_tensor_table.json, printed by tools/train_step_digest.py on that library), and every key names a parameter or
    buffer of the drop-in model with that many elements."""
    from ctc_attention_mispronunciation_amd.train import TrainHandle
    geom = synth.Geometry(**geom)
    h = TrainHandle(_config(geom), 0)
    got = [[k, n, int(b)] for k, n, b in zip(h.keys, h.numel, h.is_buffer)]
    assert got == jload("train_tensor_table.json")[name]
    model = _train_model(geom, synth.synth_state_dict(geom, seed=1))
    named = dict(model.named_parameters())
    bufs = dict(model.named_buffers())
    for k, n, b in got:
        t = bufs[k] if b else named[k]
        assert t.numel() == n, k
