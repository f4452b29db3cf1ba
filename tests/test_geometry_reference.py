"""The CPU side of tests/geometry_cases.py (no GPU): every geometry of both tables through oracle/ref_port in float32 and float64, the
expected-plan entries against csrc/plan.h itself, and the geometry contract of include/mdd_hip.h (what mdd_create and mdd_train_create
accept, the canonical-length rule) against the code that enforces it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import geometry_cases as gc
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "ctc-attention-mispronunciation_amd", "csrc")
ALL = dict(gc.DECODE, **gc.DECODE_LIMIT_EXTRA)
ALL.update({"train_" + k: (v[0], None) for k, v in gc.TRAIN.items()})


@pytest.mark.parametrize("name", sorted(ALL))
def test_reference_fp32_agrees_with_fp64_on_every_geometry(name):
    """ref_port.forward walks the state_dict's keys, so it runs every geometry as it is.  ATen's fp32 within 1e-5 of the float64 run at
    the small shape: the yardstick of the GPU tests has ten times the headroom their 1e-4 assumes; and exp(logp) sums to 1."""
    from oracle import ref_port
    from ctc_attention_mispronunciation_amd import synth
    torch.set_num_threads(min(8, torch.get_num_threads()))
    geom = gc.geometry(ALL[name][0])
    sd = synth.synth_state_dict(geom, seed=1234)
    x, x1 = gc.draw_batch(geom, *gc.SMALL, seed=5)
    assert x1.max() == geom.emb_rows - 1 and x1.min() >= 0
    t64 = {}
    l64 = ref_port.forward(sd, x, x1, dtype=torch.float64, taps=t64).numpy()
    l32 = ref_port.forward(sd, x, x1).numpy()
    assert l64.dtype == np.float64 and l64.shape == (gc.SMALL[1] // 2, gc.SMALL[0], geom.num_class)
    assert sorted(t64) == sorted(["conv1", "text", "key"] + ["rnn%d" % i for i in range(geom.layers)])
    assert t64["conv1"].shape[-1] == geom.rnn_in
    err = float(np.abs(l32.astype(np.float64) - l64).max())
    print("%s: max|fp32 - fp64| = %.3e" % (name, err))
    assert err <= 1e-5, (name, err)
    assert float(np.abs(np.exp(l64).sum(-1) - 1).max()) < 1e-12


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
        const char *why = geometry_error(c);
        if (why) { std::cout << "refused " << why << '\n'; continue; }
        const ForwardPlan p = plan_forward(c, mode, sw, fit, B);
        std::cout << p.precision << ' ' << (p.conv == Conv::Separate ? "sep" : "fused") << ' ' << (p.gated ? "layer" : "step") << ' '
                  << (mfma_tail(c) ? "mfma" : "scalar") << ' ' << max_canonical_len(c) << '\n';
    }
}
'''
_MODE = {"f32": 0, "bf16x3": 1, "f32x6": 2}
_NAME = {v: k for k, v in _MODE.items()}


def _line(g, mode=2, B=3):
    return "%d %d %d %d %d %d %d %d %d" % (g.feat, g.hidden, g.layers, g.num_class, g.channels, g.emb_rows, g.emb_dim, mode, B)


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
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


def test_expected_plans_follow_plan_h(plan_driver):
    """Every expected-plan entry of the decode table is what plan_forward gives the geometry at both batch sizes the GPU tests use; and
    which attention tail each geometry gets, with the canonical-length limits the GPU tests walk up to."""
    rows = [(n, p, B) for n in sorted(dict(gc.DECODE, **gc.DECODE_LIMIT_EXTRA)) for p in gc.PRECISIONS for B in (gc.SMALL[0], gc.WIDE[0])]
    out = plan_driver([_line(gc.decode_geometry(n), _MODE[p], B) for n, p, B in rows])
    for (n, p, B), got in zip(rows, out):
        want = (gc.DECODE.get(n) or gc.DECODE_LIMIT_EXTRA[n])[1][p]
        prec, conv, lstm, tail, lmax = got.split()
        assert (_NAME[int(prec)], conv, lstm) == want, (n, p, B, got)
        g = gc.decode_geometry(n)
        assert tail == ("mfma" if g.hidden % 64 == 0 and g.num_class <= 48 else "scalar"), (n, got)
        if n in gc.LIMIT:
            assert int(lmax) == gc.LIMIT[n], (n, got)
    assert gc.LIMIT == {"H128_L2": 2108, "H128_L2_C49": 1999}
    # the table reaches every combination the policy can produce for a geometry on a whole device
    seen = {tuple(sorted(plan.items())) for _, plan in gc.DECODE.values()}
    assert len(seen) == 6


REFUSED = [
    (dict(feat=2), "feat"), (dict(hidden=0), "hidden"), (dict(hidden=-4), "hidden"), (dict(hidden=18), "hidden"), (dict(hidden=1028), "hidden"),
    (dict(layers=0), "layers"), (dict(num_class=1), "num_class"), (dict(channels=8), "channels"), (dict(channels=0), "channels"),
    (dict(emb_rows=0), "emb_rows"), (dict(emb_dim=10), "emb_dim"), (dict(emb_dim=0), "emb_dim"), (dict(emb_dim=510), "emb_dim"),
    # the scalar attention tail with no room for a single canonical phoneme: 4H + C >= 2560
    (dict(hidden=640, num_class=49), "attention tail"), (dict(hidden=628, num_class=48), "attention tail"), (dict(hidden=1020), "attention tail"),
]
ACCEPTED = [dict(), dict(hidden=4), dict(hidden=20), dict(hidden=1024), dict(hidden=1024, num_class=48), dict(hidden=636, num_class=15),
            dict(feat=3), dict(channels=4), dict(emb_dim=4), dict(emb_rows=1), dict(num_class=2), dict(layers=1), dict(layers=9)]


def test_geometry_contract_in_plan_h(plan_driver):
    """geometry_error, the one check both create calls make: each stated constraint refused by name just outside and accepted just inside,
    and the largest canonical length of an accepted geometry is at least 1."""
    out = plan_driver([_line(gc.geometry(k)) for k, _ in REFUSED])
    for (k, word), got in zip(REFUSED, out):
        assert got.startswith("refused ") and word in got, (k, got)
    out = plan_driver([_line(gc.geometry(k)) for k in ACCEPTED])
    for k, got in zip(ACCEPTED, out):
        assert not got.startswith("refused"), (k, got)
        assert int(got.split()[-1]) >= 1, (k, got)
    g = gc.geometry(dict(hidden=636, num_class=15))
    assert plan_driver([_line(g)])[0].split()[-2:] == ["scalar", "1"]          # 2560 - 4 * 636 - 15


def test_both_create_calls_refuse_on_the_host():
    """mdd_create and mdd_train_create return MDD_ERR_ARG for a geometry outside the contract before they touch a device, name the field
    in mdd_last_error() and leave the handle pointer alone: emb_dim = 10 (the training step never took it, the decode handle used to),
    hidden = 18, channels = 8, a hidden size past 1024, feat = 2, a classifier of one class."""
    from ctc_attention_mispronunciation_amd import _lib
    lib = _lib.lib()
    for kwargs, word in REFUSED:
        g = gc.geometry(kwargs)
        cfg = _lib.MddConfig(feat=g.feat, hidden=g.hidden, layers=g.layers, num_class=g.num_class, channels=g.channels,
                             emb_rows=g.emb_rows, emb_dim=g.emb_dim, bn_eps=1e-5)
        for create in (lib.mdd_create, lib.mdd_train_create):
            h = C.c_void_p()
            assert create(C.byref(cfg), 0, C.byref(h)) == -1, kwargs            # MDD_ERR_ARG
            msg = lib.mdd_last_error().decode()
            assert "unsupported geometry" in msg and word in msg, (kwargs, msg)
            assert not h.value


def test_header_and_readme_state_the_contract():
    """The text a user reads says what the check does: hidden a multiple of 4 (not 16), emb_dim a multiple of 4, the general L rule."""
    with open(os.path.join(ROOT, "include", "mdd_hip.h")) as f:
        header = f.read()
    assert "multiple of 16" not in header
    for phrase in ("hidden a multiple of 4, 4 <= hidden <= 1024", "emb_dim a multiple of 4", "channels 32 or 4", "feat >= 3",
                   "L <= 2364 - 2H", "L <= 2560 - 4H - C", "2108 at H = 128", "1999 at"):
        assert phrase in header, phrase
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    for phrase in ("tests/test_geometry.py", "tests/test_train_geometry.py", "tests/test_geometry_reference.py"):
        assert phrase in readme, phrase
