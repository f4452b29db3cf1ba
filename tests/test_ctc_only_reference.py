"""The CPU side of the CTC-only model (the reference's egs/cnn-rnn-ctc baseline; GPU side: tests/test_ctc_only.py): the float64 restatement
the GPU tests measure against is pinned to the reference's own output (G15), the drop-in class has the reference's state_dict, the geometry
contract and the plan of a CTC-only handle are what csrc/plan.h states, the built library has the entry points, and the synthetic weights
of the attention model are the bytes they were before the CTC-only geometry existed."""
import hashlib
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import ctc_only_cases as cc
from tests.helpers import ROOT, jload, npz

CSRC = os.path.join(ROOT, "ctc-attention-mispronunciation_amd", "csrc")


def _g15():
    return jload("g15_ctc_only.json"), npz("g15_ctc_only.npz")


@pytest.mark.parametrize("tag", ["tiny", "h256", "h384"])
def test_float64_restatement_matches_the_reference_output(tag):
    """forward_f64 on G15's inputs against the log-probs the reference's own CTC_Model gave in fp32: within 1e-4 (README's parity
    tolerance).  Measured: tiny 7.2e-7, h256 1.9e-6, h384 2.5e-6 -- the reference's fp32 rounding."""
    from ctc_attention_mispronunciation_amd import synth
    torch.set_num_threads(min(8, torch.get_num_threads()))
    meta, g = _g15()
    case = [c for c in meta["cases"] if c["tag"] == tag][0]
    geom = synth.Geometry(ctc_only=True, **case["geom"])
    sd = synth.synth_state_dict(geom, seed=case["seed"])
    x = g[tag + "_x"]
    again, _, frac, _ = synth.synth_batch(geom, B=meta["B"], T=meta["T"], L=meta["L"], seed=case["batch_seed"])
    np.testing.assert_array_equal(again, x)             # the recorded inputs are the seeded ones
    np.testing.assert_array_equal(frac, g[tag + "_frac"])
    l64 = cc.forward_f64(sd, x)
    ref = g[tag + "_logp"]
    assert l64.dtype == np.float64 and ref.dtype == np.float32 and l64.shape == ref.shape == (meta["T"] // 2, meta["B"], geom.num_class)
    err = float(np.abs(l64 - ref.astype(np.float64)).max())
    print("%s: max|float64 restatement - reference fp32| = %.3e" % (tag, err))
    assert err <= cc.TOL, (tag, err)
    assert float(np.abs(np.exp(l64).sum(-1) - 1).max()) < 1e-12
    # the tail alone, from the restatement's own last-layer output, is the same function
    taps = {}
    cc.forward_f64(sd, x, taps=taps)
    np.testing.assert_allclose(cc.tail_f64(sd, taps["rnn%d" % (geom.layers - 1)]), l64, rtol=0, atol=1e-12)


@pytest.mark.parametrize("tag", ["tiny", "h384"])
def test_drop_in_state_dict_is_the_reference_list(tag):
    """models.cnn_rnn.CTC_Model().state_dict(): the float keys, their order and shapes equal the reference model's (G15), at 2 and 4
    layers; 12 + 4 layers + 4 (layers - 1) + 5 of them; and synth_state_dict gives exactly that list."""
    import torch.nn as nn
    from ctc_attention_mispronunciation_amd import synth
    from ctc_attention_mispronunciation_amd.models import cnn_rnn, model_ctc
    meta, _ = _g15()
    case = [c for c in meta["cases"] if c["tag"] == tag][0]
    geom = synth.Geometry(ctc_only=True, **case["geom"])
    assert geom.emb_rows == 0 and geom.emb_dim == 0 and geom.ctc_only
    model = cnn_rnn.CTC_Model(add_cnn=True, cnn_param=geom.cnn_param(nn), rnn_param=geom.rnn_param(nn), num_class=geom.num_class, drop_out=0.2)
    assert isinstance(model, model_ctc.CTC_Model) and cnn_rnn.BatchRNN is model_ctc.BatchRNN      # shared containers, not copies
    got = [[k, list(v.shape)] for k, v in model.state_dict().items() if v.is_floating_point()]
    assert got == case["keys"]
    assert len(got) == 12 + 4 * geom.layers + 4 * (geom.layers - 1) + 5 == {2: 29, 4: 45}[geom.layers]
    sd = synth.synth_state_dict(geom, seed=3)
    assert [[k, list(v.shape)] for k, v in sd.items() if v.dtype.kind == "f"] == case["keys"]
    assert not any(k.startswith(("embeds", "lstm_embeds", "score")) for k in sd)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})             # strict
    # the attention class is what it was
    att = synth.Geometry(**synth.TINY)
    assert not att.ctc_only and (att.emb_rows, att.emb_dim) == (7, 12)
    full = model_ctc.CTC_Model(add_cnn=True, cnn_param=att.cnn_param(nn), rnn_param=att.rnn_param(nn), num_class=att.num_class)
    assert "embeds.weight" in full.state_dict() and full.state_dict()["fc.1.weight"].shape == (att.num_class, 4 * att.hidden)
    with pytest.raises(NotImplementedError, match="CTC-only training is not built"):
        model.train()(torch.zeros(1, 4, geom.feat), None)


_DRIVER = r'''
#include <iostream>
#include <sstream>
#include <string>
#include "plan.h"
using namespace mdd;
// stdin, one case per line: feat hidden layers num_class channels emb_rows emb_dim mode B
int main() {
    const Switches sw;                                  // no environment switch
    const DeviceFit fit{true, true, true};              // a whole MI355X holds every persistent grid
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        mdd_config c{};
        int mode, B;
        in >> c.feat >> c.hidden >> c.layers >> c.num_class >> c.channels >> c.emb_rows >> c.emb_dim >> mode >> B;
        c.bn_eps = 1e-5f;
        const char *why = ctc_geometry_error(c);
        if (why) { std::cout << "refused " << why << '\n'; continue; }
        const ForwardPlan p = plan_forward(c, mode, sw, fit, B, true);
        mdd_config a = c;                               // the attention handle of the same acoustic geometry, reference text side
        a.emb_rows = 44; a.emb_dim = 512;
        const ForwardPlan q = plan_forward(a, mode, sw, fit, B);
        const bool same = p.precision == q.precision && p.conv == q.conv && p.proj == q.proj && p.lstm == q.lstm && p.gated == q.gated &&
                          p.hx_floats == q.hx_floats && p.stamps_at == q.stamps_at && p.planes_out == q.planes_out;
        std::cout << p.precision << ' ' << (p.text_table ? "table" : "notable") << ' ' << (mfma_ctc_tail(c) ? "mfma" : "scalar") << ' '
                  << (same ? "same" : "differs") << ' ' << (geometry_error(c) ? "attention-refuses" : "attention-accepts") << '\n';
    }
}
'''


def _line(g, mode=2, B=3, **over):
    v = dict(feat=g.feat, hidden=g.hidden, layers=g.layers, num_class=g.num_class, channels=g.channels, emb_rows=g.emb_rows, emb_dim=g.emb_dim)
    v.update(over)
    return "%d %d %d %d %d %d %d %d %d" % (v["feat"], v["hidden"], v["layers"], v["num_class"], v["channels"], v["emb_rows"], v["emb_dim"], mode, B)


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("ctc_plan")
    (d / "drv.cpp").write_text(_DRIVER)
    exe = str(d / "drv")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "drv.cpp"), "-o", exe])

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


REFUSED = [(dict(emb_rows=44), "emb_rows"), (dict(emb_rows=1), "emb_rows"), (dict(emb_dim=512), "emb_dim"), (dict(emb_dim=4), "emb_dim"),
           (dict(emb_rows=44, emb_dim=512), "emb_rows"),
           # the other fields as in the attention contract (tests/test_geometry_reference.py), the same words
           (dict(feat=2), "feat"), (dict(hidden=0), "hidden"), (dict(hidden=18), "hidden"), (dict(hidden=1028), "hidden"), (dict(layers=0), "layers"),
           (dict(num_class=1), "num_class"), (dict(channels=8), "channels")]
# ... and no attention-tail room condition: 4H + C >= 2560 is accepted here
ACCEPTED = [dict(), dict(hidden=4), dict(hidden=20), dict(hidden=1024), dict(hidden=640, num_class=49), dict(hidden=1020), dict(feat=3),
            dict(channels=4), dict(num_class=2), dict(num_class=300), dict(layers=1), dict(layers=9)]


def test_ctc_geometry_contract_in_plan_h(plan_driver):
    """ctc_geometry_error: emb_rows / emb_dim other than 0 refused by name, the shared fields refused as the attention contract refuses
    them, the attention tail's room condition gone; mdd_create's contract still refuses emb_rows = 0."""
    g = cc.geometry({})
    out = plan_driver([_line(g, **k) for k, _ in REFUSED])
    for (k, word), got in zip(REFUSED, out):
        assert got.startswith("refused ") and word in got, (k, got)
    out = plan_driver([_line(cc.geometry(k)) for k in ACCEPTED])
    for k, got in zip(ACCEPTED, out):
        assert not got.startswith("refused"), (k, got)
        assert got.split()[-1] == "attention-refuses", (k, got)          # emb_rows = 0 is no geometry of mdd_create
    with open(os.path.join(ROOT, "include", "mdd_hip.h")) as f:
        header = f.read()
    for phrase in ("mdd_create_ctc", "mdd_is_ctc_only", "emb_rows = 0 and emb_dim = 0", "ctc_geometry_error, csrc/plan.h"):
        assert phrase in header, phrase


def test_ctc_plan_table_in_plan_h(plan_driver):
    """plan_forward for a CTC-only handle: never a text table; emb_dim (0) plays no part in the mode fallbacks, so every mode, kernel
    choice and exchange-buffer size is that of the attention handle with the same acoustic geometry and a reference text side; the
    fallbacks are the documented ones (tests/ctc_only_cases.expected_precision); the tail form follows the stated rule."""
    names = dict(cc.CASES, **cc.LAYER_CASES)
    rows = [(n, p, B) for n in sorted(names) for p in cc.MODES for B in (3, 17, 200)]
    out = plan_driver([_line(cc.geometry(names[n][0]), cc.MODES[p], B) for n, p, B in rows])
    inv = {v: k for k, v in cc.MODES.items()}
    for (n, p, B), got in zip(rows, out):
        g = cc.geometry(names[n][0])
        prec, table, tail, same, _ = got.split()
        assert inv[int(prec)] == cc.expected_precision(g, p), (n, p, got)
        assert table == "notable" and same == "same", (n, p, B, got)
        assert tail == names[n][1] == cc.tail_form(g), (n, got)
    # every mode is honoured at the two recipe geometries, and each fallback occurs
    assert cc.expected_precision(cc.geometry({}), "bf16x3") == "bf16x3" and cc.expected_precision(cc.geometry(dict(hidden=256)), "f32x6") == "f32x6"
    assert cc.expected_precision(cc.geometry(cc.CASES["H128_C45"][0]), "bf16x3") == "f32"
    assert cc.expected_precision(cc.geometry(cc.CASES["tiny"][0]), "f32x6") == "f32"


def test_library_exports_the_ctc_only_entry_points():
    """The built library has mdd_create_ctc and mdd_is_ctc_only, the binding lists them, and mdd_create_ctc refuses a geometry with an
    embedding on the host, naming the field, before it touches a device."""
    import ctypes as C
    from ctc_attention_mispronunciation_amd import _lib
    lib = _lib.lib()
    for name in ("mdd_create_ctc", "mdd_is_ctc_only"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    cfg = _lib.MddConfig(feat=243, hidden=384, layers=4, num_class=45, channels=32, emb_rows=44, emb_dim=0, bn_eps=1e-5)
    h = C.c_void_p()
    assert lib.mdd_create_ctc(C.byref(cfg), 0, C.byref(h)) == -1 and not h.value
    msg = lib.mdd_last_error().decode()
    assert "mdd_create_ctc" in msg and "emb_rows" in msg, msg
    assert lib.mdd_is_ctc_only(None) == 0


def _digest(kw, seed, **opts):
    from ctc_attention_mispronunciation_amd import synth
    geom = synth.Geometry(**kw)
    h = hashlib.sha256()
    for k, v in synth.synth_state_dict(geom, seed=seed, **opts).items():
        a = np.ascontiguousarray(v)
        h.update(k.encode()); h.update(str(a.dtype).encode()); h.update(str(a.shape).encode()); h.update(a.tobytes())
    for a in synth.synth_batch(geom, B=3, T=12, L=5, seed=seed):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_attention_synthetic_weights_are_unchanged():
    """synth_state_dict and synth_batch of a geometry that is not CTC-only: keys, dtypes, shapes and bytes digest to what the code before
    the CTC-only geometry gave (the digests were computed on that code): the goldens regenerate their weights from seeds."""
    from ctc_attention_mispronunciation_amd import synth
    assert _digest(synth.REFERENCE, 1234) == "2834d22b0da15ee9f36c6b3dafc8d339c0899c61425591c88b9183f07316543c"
    assert _digest(synth.TINY, 7) == "527984c5b2f5f59d58e5f82bb291e8ca6d15acff0c3a7f34bd8daab9511de9b2"
    assert _digest(synth.REFERENCE_256, 11, score_gain=16.0) == "889e1287c2a15aa44b478f4054a154ad67a37c7fef20832032974db76c202b3b"
