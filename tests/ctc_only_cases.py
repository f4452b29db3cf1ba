"""Helpers of the CTC-only model's tests (tests/test_ctc_only_reference.py on the CPU, tests/test_ctc_only.py on the GPU); no tests here.

* ``forward_f64``: the eval forward of the reference's CTC-only baseline model (CRC/models/cnn_rnn.py:147-179) restated in torch ops and
  evaluated in float64 from a state_dict -- conv x 2 (k3, strides (1,2) and (2,2), pad 1, BatchNorm2d, ReLU), ``layers`` x BiLSTM without
  bias (BatchNorm1d in front of every layer but the first), BatchNorm1d(2H) + Linear(2H -> C, no bias), log-softmax.  Dropout is the
  identity in eval mode.  tests/test_ctc_only_reference.py pins it to the reference's own fp32 output (tests/golden/g15_ctc_only.*).
* ``tail_f64``: the last three steps alone, from given last-layer outputs.
* ``draw_batch``: features with ragged zero padding, as the collate pads.
* ``CASES``: geometry name -> (Geometry kwargs, the form of ctc_tail it must get).  ``SHAPES``: the (B, T) of the tail's row edges.
"""
import numpy as np
import torch
import torch.nn.functional as F

from ctc_attention_mispronunciation_amd import synth

TOL = 1e-4      # README's parity tolerance
MODES = {"f32": 0, "bf16x3": 1, "f32x6": 2}

TINY_CTC = dict(feat=15, hidden=8, layers=2, num_class=7, channels=4)
# name -> (Geometry kwargs over the reference's defaults, tail form).  Matrix-core form: 2H % 64 == 0 and C <= 48 (csrc/plan.h, mfma_ctc_tail).
CASES = {
    "H384": (dict(), "mfma"),
    "H256": (dict(hidden=256), "mfma"),
    "H64_C48": (dict(hidden=64, layers=2, num_class=48), "mfma"),         # J = 2H / 16 = 8: two passes of the K loop; the last class of the third tile
    "H128_C45": (dict(hidden=128, layers=2), "mfma"),
    "H128_C49": (dict(hidden=128, layers=2, num_class=49), "scalar"),     # one class past the three tiles
    "H20_ch4_C12_feat39": (dict(feat=39, hidden=20, layers=2, channels=4, num_class=12), "scalar"),   # 2H = 40: ten lanes hold a row
    "H256_C2": (dict(hidden=256, layers=1, num_class=2), "mfma"),
    "H256_C101": (dict(hidden=256, layers=1, num_class=101), "scalar"),   # two logits per lane
    "tiny": (TINY_CTC, "scalar"),
}
# (C = 2 is within the matrix-core form's rule: one live column in the first of its three tiles)
LAYER_CASES = {"H256_L1": (dict(hidden=256, layers=1), "mfma"), "H256_L6": (dict(hidden=256, layers=6), "mfma")}
# (B, T): R = T/2 * B = 21 (a partial 16-row tile), 561 (no multiple of 16 or 64, nine workgroups of the matrix-core form), 1 (the smallest)
SHAPES = ((3, 14), (17, 66), (1, 2))


def geometry(kwargs):
    return synth.Geometry(ctc_only=True, **dict(synth.REFERENCE, **kwargs))


def tail_form(geom):
    return "mfma" if (2 * geom.hidden) % 64 == 0 and geom.num_class <= 48 else "scalar"


def expected_precision(geom, asked):
    """The mode in effect (include/mdd_hip.h at mdd_set_precision, with emb_dim taking no part): modes 1 and 2 need the contraction
    lengths channels x W2 and (mode 2) 2H to be multiples of 32, mode 1 also H in {256, 384}; mode 0 otherwise."""
    k0 = geom.rnn_in % 32 == 0
    if asked == "f32x6" and k0 and (2 * geom.hidden) % 32 == 0:
        return "f32x6"
    if asked == "bf16x3" and k0 and geom.hidden in (256, 384):
        return "bf16x3"
    return "f32"


def draw_batch(geom, B, T, seed):
    """x [B, T, feat] float32 N(0, 1); every row but the first zero from a random even length >= T/2 on."""
    rng = np.random.Generator(np.random.PCG64(seed + 17))
    x = rng.standard_normal((B, T, geom.feat)).astype(np.float32)
    for b in range(1, B):
        tb = int(rng.integers(T // 2, T + 1))
        tb -= tb % 2
        x[b, tb:, :] = 0.0
    return x


def _t(sd, key, dtype):
    return torch.from_numpy(np.asarray(sd[key])).to(dtype)


def _bn(sd, prefix, v, dtype, eps=1e-5):
    """eval-mode BatchNorm over the channel axis 1 of v"""
    return F.batch_norm(v, _t(sd, prefix + ".running_mean", dtype), _t(sd, prefix + ".running_var", dtype), _t(sd, prefix + ".weight", dtype),
                        _t(sd, prefix + ".bias", dtype), training=False, eps=eps)


def tail_f64(sd, h):
    """log_softmax(Linear(BatchNorm1d(h))) in float64: h [T', B, 2H] (any float dtype) -> [T', B, C]"""
    dt = torch.float64
    h = torch.as_tensor(h).to(dt)
    Tp, B, K = h.shape
    y = _bn(sd, "fc.0", h.reshape(Tp * B, K), dt)
    return F.log_softmax(F.linear(y, _t(sd, "fc.1.weight", dt)).view(Tp, B, -1), dim=-1).numpy()


def forward_f64(sd, x, dtype=torch.float64, taps=None):
    """x [B, T, feat] -> log-probs [T/2, B, C] as a numpy array of `dtype`.  taps (dict): "conv1" and "rnn<i>" (raw layer outputs)."""
    layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("rnns."))
    with torch.no_grad():
        v = torch.from_numpy(np.asarray(x)).to(dtype).unsqueeze(1)                               # [B, 1, T, F]
        for n, stride in ((0, (1, 2)), (1, (2, 2))):
            v = F.conv2d(v, _t(sd, "conv.%d.conv.weight" % n, dtype), _t(sd, "conv.%d.conv.bias" % n, dtype), stride=stride, padding=(1, 1))
            v = torch.relu(_bn(sd, "conv.%d.batch_norm" % n, v, dtype))
        B, ch, Tp, W = v.shape
        v = v.transpose(1, 2).contiguous().view(B, Tp, ch * W).transpose(0, 1).contiguous()       # [T', B, ch * W2]
        if taps is not None:
            taps["conv1"] = v.numpy().copy()
        for n in range(layers):
            if n > 0:
                v = _bn(sd, "rnns.%d.batch_norm" % n, v.transpose(-1, -2), dtype).transpose(-1, -2)   # over the feature axis, as cnn_rnn.py:29-32
            H = np.asarray(sd["rnns.%d.rnn.weight_hh_l0" % n]).shape[1]
            rnn = torch.nn.LSTM(input_size=v.shape[-1], hidden_size=H, bidirectional=True, bias=False).to(dtype)
            rnn.load_state_dict({k: _t(sd, "rnns.%d.rnn.%s" % (n, k), dtype) for k in
                                 ("weight_ih_l0", "weight_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse")})
            v, _ = rnn(v.contiguous())
            if taps is not None:
                taps["rnn%d" % n] = v.numpy().copy()
        y = _bn(sd, "fc.0", v.reshape(Tp * B, -1), dtype)
        return F.log_softmax(F.linear(y, _t(sd, "fc.1.weight", dtype)).view(Tp, B, -1), dim=-1).numpy()


def attention_twin(geom_ctc, sd_ctc, seed):
    """An attention geometry and state_dict with the CTC-only model's conv and BiLSTM weights: (Geometry, state_dict)."""
    kw = dict(feat=geom_ctc.feat, hidden=geom_ctc.hidden, layers=geom_ctc.layers, num_class=geom_ctc.num_class, channels=geom_ctc.channels)
    if geom_ctc.hidden == 8:
        kw.update(emb_rows=7, emb_dim=12)     # synth.TINY's text side
    geom = synth.Geometry(**kw)
    sd = synth.synth_state_dict(geom, seed=seed)
    for k, v in sd_ctc.items():
        if k.startswith("conv.") or k.startswith("rnns."):
            assert sd[k].shape == v.shape
            sd[k] = v
    return geom, sd
