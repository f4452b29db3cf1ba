"""The CPU side of tests/batch_tile_cases.py (no GPU): the hand-made NBT table against csrc/plan.h itself, the float64 yardstick at the
large batches (ATen's fp32 run stays within 1e-5 of it; the reference has no cross-batch operation, so the small-batch pins of the
goldens extend to any B), and the training shapes of tests/test_train_batch_tiles.py through oracle/ref_port.train_step in float64."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import batch_tile_cases as bt
from tests import geometry_cases as gc
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "ctc-attention-mispronunciation_amd", "csrc")

_DRIVER = r'''
#include <iostream>
#include <sstream>
#include <string>
#include "plan.h"
using namespace mdd;
// stdin, one case per line: hidden mode B force        (reference geometry otherwise; force: MDD_LSTM_X6=force)
// stdout: team8_tiles(B), x6_tiles(B), the recurrence plan_forward picks, gated, the mode, kPersistMaxB, the two families' largest tile counts
int main() {
    const DeviceFit fit{true, true, true};              // a whole MI355X holds every persistent grid
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        mdd_config c{};
        int mode, B, force;
        in >> c.hidden >> mode >> B >> force;
        c.feat = 243; c.layers = 4; c.num_class = 45; c.channels = 32; c.emb_rows = 44; c.emb_dim = 512; c.bn_eps = 1e-5f;
        if (geometry_error(c)) return 2;
        Switches sw;
        sw.x6_force = force != 0;
        const ForwardPlan p = plan_forward(c, mode, sw, fit, B);
        const char *lstm = p.lstm == Lstm::X6 ? "x6" : p.lstm == Lstm::F32 ? "f32" : p.lstm == Lstm::Granule ? "granule" : "step";
        std::cout << team8_tiles(B) << ' ' << x6_tiles(B) << ' ' << lstm << ' ' << (p.gated ? 1 : 0) << ' ' << p.precision << ' ' << kPersistMaxB << ' '
                  << kTeam8MaxTiles << ' ' << kX6MaxTiles << '\n';
    }
}
'''
_MODE = {"f32": 0, "bf16x3": 1, "f32x6": 2}


@pytest.fixture(scope="module")
def tile_driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("tiles")
    (d / "drv.cpp").write_text(_DRIVER)
    exe = str(d / "drv")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "drv.cpp"), "-o", exe])

    def run(rows):
        r = subprocess.run([exe], input="".join("%d %d %d %d\n" % row for row in rows), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = r.stdout.splitlines()
        assert len(out) == len(rows)
        return [o.split() for o in out]
    return run


def test_nbt_table_follows_plan_h(tile_driver):
    """The hand-made NBT table is team8_tiles(B) and x6_tiles(B) of csrc/plan.h (ceil(ceil(B / 16) / 16) and ceil(ceil(B / 8) / 16)); the layer kernel each (H, precision) is
    expected to run at the TILE_B batches is plan_forward's choice, MDD_LSTM_X6=force gives the f32x6 teams at H = 256, and B = 1025 gets no
    layer kernel in any mode.  Every instantiation NBT = 1..8 (x6) and 1..4 (granule, f32) occurs for both hidden sizes."""
    assert bt.TILE_B == (129, 257, 385, 513, 641, 769, 897, 1024) and bt.PAST_B == 1025 and bt.LONG[1] == 300
    batches = sorted(bt.NBT)
    assert set(batches) == set(bt.TILE_B) | {17, bt.LONG[1], bt.PAST_B}
    for H in bt.HIDDEN:
        for p in bt.PRECISIONS:
            got = tile_driver([(H, _MODE[p], B, 0) for B in batches])
            for B, (team8, x6, lstm, gated, prec, max_b, max_team8, max_x6) in zip(batches, got):
                assert int(max_b) == 1024 and int(prec) == _MODE[p] and (int(max_team8), int(max_x6)) == (4, 8)
                want_x6, want_team8 = bt.NBT[B]
                if B > 1024:
                    assert (want_x6, want_team8) == (None, None) and (lstm, gated) == ("step", "0"), (H, p, B, lstm)
                    continue
                assert (int(x6), int(team8)) == (want_x6, want_team8), (H, B, x6, team8)
                assert (int(x6), int(team8)) == (-(-(-(-B // 8)) // 16), -(-(-(-B // 16)) // 16)), B
                assert gated == "1"
                if B > 128:
                    assert lstm == bt.LAYER_KERNEL[H, p], (H, p, B, lstm)
                else:           # B = 17: the f32x6 teams at either hidden size
                    assert lstm == ("x6" if p == "f32x6" else bt.LAYER_KERNEL[H, p]), (H, p, B, lstm)
        forced = tile_driver([(H, _MODE["f32x6"], B, 1) for B in bt.TILE_B])
        assert [f[2] for f in forced] == ["x6"] * len(bt.TILE_B), (H, forced)
    # every batch up to kPersistMaxB stays within both families' largest instantiation, and kPersistMaxB is the largest that does
    every = tile_driver([(384, _MODE["f32x6"], B, 0) for B in range(1, 1026)])
    for B, (team8, x6, _, _, _, max_b, max_team8, max_x6) in zip(range(1, 1026), every):
        assert (1 <= int(team8) <= int(max_team8) and 1 <= int(x6) <= int(max_x6)) == (B <= int(max_b)), (B, team8, x6)
    assert int(every[-1][0]) > 4 and int(every[-1][1]) > 8
    # which instantiations the batches reach (B = 17: tests/test_geometry.py; 300: the long case; the rest: TILE_B)
    on = [B for B in batches if B <= 1024]
    assert sorted({bt.NBT[B][0] for B in on}) == list(range(1, 9))
    assert sorted({bt.NBT[B][1] for B in on}) == list(range(1, 5))
    assert [bt.NBT[B][1] for B in bt.TILE_B] == [1, 2, 2, 3, 3, 4, 4, 4]
    assert [bt.NBT[B][0] for B in bt.TILE_B] == [2, 3, 4, 5, 6, 7, 8, 8]
    assert bt.NBT[bt.LONG[1]] == (3, 2)
    assert set(bt.LAYER_KERNEL) == {(H, p) for H in bt.HIDDEN for p in bt.PRECISIONS}


@pytest.mark.parametrize("H,B", [(384, 1024), (256, 513)])
def test_yardstick_is_sound_at_large_batches(H, B):
    """ATen's fp32 run of the reference graph within 1e-5 of the float64 run on log-probs and every tap (the bound of
    tests/test_geometry_reference.py, ten times inside the GPU tests' 1e-4), at a full-size and a ragged-tile batch; and rows 0, 128, 129
    and B - 1 of the float64 run equal the float64 run of those four utterances alone within 1e-12: no operation of the eval-mode graph
    crosses the batch, so what the goldens pin at small batches holds at any B."""
    from oracle import ref_port
    x, x1, logp, taps = bt.case(H, B)
    geom = bt.geometry(H)
    assert logp.shape == (bt.SHORT[0] // 2, B, geom.num_class)
    assert sorted(taps) == sorted(bt.tap_names(geom))
    d32 = bt.aten_fp32_distance(H, B)
    print("H=%d B=%d: max|fp32 - fp64| " % (H, B) + " ".join("%s %.2e" % kv for kv in sorted(d32.items())))
    assert sorted(d32) == sorted(["logp"] + [k for k in taps if k != "score"])
    for k, e in d32.items():
        assert e <= 1e-5, (H, B, k, e)
    assert float(np.abs(np.exp(logp).sum(-1) - 1).max()) < 1e-12
    rows = [0, 128, 129, B - 1]
    t4 = {}
    l4 = ref_port.forward(bt.state_dict(H), x[rows], x1[rows], dtype=torch.float64, taps=t4).numpy()
    t4["score"] = gc.reference_scores(t4, geom.layers)
    assert float(np.abs(l4 - logp[:, rows]).max()) <= 1e-12
    for k, v in t4.items():
        whole = taps[k][rows] if k == "score" else taps[k][:, rows]        # score is [B, T', L], every other tap [., B, .]
        assert v.shape == whole.shape, (k, v.shape, whole.shape)
        assert float(np.abs(v - whole).max()) <= 1e-12, k


@pytest.mark.parametrize("H,B,T,L", bt.TRAIN_SHAPES)
def test_training_shapes_are_feasible(H, B, T, L):
    """Every shape of tests/test_train_batch_tiles.py gives a finite float64 loss (each row's CTC alignment exists at T' = 4) and finite
    gradients for every parameter, and the batch statistics cover at least 64 rows."""
    assert B * T >= 64
    geom, (sd, x, x1, masks, tg, il, tl), (logp, loss, grads, run) = bt.train_case(H, B, T, L)
    assert logp.shape == (T // 2, B, geom.num_class) and np.isfinite(logp).all()
    assert np.isfinite(loss) and 0 < loss < 1e3, loss
    assert int(il.min()) >= 1 and int(il.max()) <= T // 2 and int(tl.min()) >= 1
    assert set(grads) == {k for k, v in sd.items() if np.asarray(v).dtype.kind == "f" and "running_" not in k}
    for k, g in grads.items():
        assert np.isfinite(g).all(), k
    assert any(float(np.abs(g).max()) > 0 for g in grads.values())
    for k, v in run.items():
        assert np.isfinite(v).all(), k
