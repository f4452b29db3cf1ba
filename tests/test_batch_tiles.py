"""The decode forward in every batch-tile geometry of the persistent BiLSTM layer kernels (GPU), against oracle/ref_port.forward in
float64 -- an outside reference, where every other test past 64 rows compares one kernel of the library with another.

RUNS walks tests/batch_tile_cases.py: every B of TILE_B (the first batch of each lstm_layer_x6_kernel<H, 2..8> and B = 1024; granule / f32
tiles 1, 2, 2, 3, 3, 4, 4, 4) at H = 384 and 256 in the three precisions; MDD_LSTM_X6=force at H = 256 (the library's own choice gives
those batches to the exact-fp32 layer kernel, so lstm_layer_x6_kernel<256, 2..8> is anchored only here); B = 1025, where every mode falls
back to one launch per step; the per-step kernels themselves at B = 129 and 1024 (MDD_LSTM=step in mode f32, MDD_LSTM=x3 in mode bf16x3:
the yardsticks of the bitwise persistent-against-step tests); handles without taps at B = 513 (the default f32x6 layers then write bf16
planes and no fp32 copy); and one long recurrence, T' = 60 at B = 300 (x6: three tiles per team on the skewed schedule, granule / f32: two).

Per run: the precision in effect and the launch counts of HipModel.profile say which path ran; conv1, rnn0..3, text, key, score and the
log-probs are each within the project's 1e-4 of float64, compared in forward order; rows sum to 1; the graph replay gives the same bits.
The two reference-width modes are held tighter on the log-probs and the rnn taps: at most max(4 d32, 2e-6), d32 being ATen's own fp32
distance to float64 for the same tensor of the same case (it comes from the reference, not from the code under test; 4 is a margin over
the 2x and 1.25x of test_error_against_fp64_beside_aten_fp32, the ratio of two rounding-level quantities being noisier at T' = 6; a lost
mid or lo plane or a wrong row is 100x or more).  Distances and ratios are recorded under "tiles_" / "tiles_ratio_"; the GPU run's values
are committed as profiles/batch_tiles_margins.json."""
import numpy as np
import pytest
import torch

from tests import batch_tile_cases as bt
from tests.helpers import record_margin

pytestmark = pytest.mark.gpu
TOL = 1e-4
RATIO, FLOOR = 4.0, 2e-6
SWITCH = {None: None, "x6force": ("MDD_LSTM_X6", "force"), "step": ("MDD_LSTM", "step"), "x3": ("MDD_LSTM", "x3")}


def _runs():
    """(H, B, T, L, precision, switch, taps), the runs of one (H, B, T, L) next to each other: they share its float64 case."""
    T, L = bt.SHORT
    runs = []
    for H in bt.HIDDEN:
        for B in bt.TILE_B:
            runs += [(H, B, T, L, p, None, True) for p in bt.PRECISIONS]
            if H == 256:
                runs.append((H, B, T, L, "f32x6", "x6force", True))
            if B in (129, 1024):
                runs += [(H, B, T, L, "f32", "step", True), (H, B, T, L, "bf16x3", "x3", True)]
            if (H, B) == (384, 513):
                runs += [(H, B, T, L, p, None, False) for p in bt.PRECISIONS]
        runs += [(H, bt.PAST_B, T, L, p, None, True) for p in bt.PRECISIONS]
    runs += [bt.LONG + (p, None, True) for p in bt.PRECISIONS]
    return runs


RUNS = _runs()


def _id(run):
    H, B, T, L, precision, switch, taps = run
    return "-".join(["H%d" % H, "B%d" % B] + (["T%d" % T] if T != bt.SHORT[0] else []) + [precision] + ([switch] if switch else []) + ([] if taps else ["notaps"]))


def _hip():
    from ctc_attention_mispronunciation_amd import hip_model
    return hip_model


def _cuda(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()      # (the cached cases are read-only)


def _expected_kernel(H, B, precision, switch):
    """"x6" | "f32" | "granule": one persistent launch per BiLSTM; "step": one launch per time step."""
    if B > 1024 or switch in ("step", "x3"):
        return "step"
    return "x6" if switch == "x6force" else bt.LAYER_KERNEL[H, precision]


def _assert_path(m, run, x, x1):
    """The observables of the path the case is about: the precision in effect and the recurrences' launch counts."""
    H, B, T, L, precision, switch, _ = run
    assert m.precision == precision, (run, m.precision)
    launches = {n: l for n, _, l, _ in m.profile(x, x1)}
    layer = _expected_kernel(H, B, precision, switch) != "step"
    for n in range(m.geom.layers):
        assert launches["lstm%d" % n] == (1 if layer else T // 2), (run, n, launches)
    assert launches["lstm_text"] == (1 if layer else L), (run, launches)


@pytest.mark.parametrize("run", RUNS, ids=[_id(r) for r in RUNS])
def test_forward_tiles_against_float64(run, monkeypatch):
    H, B, T, L, precision, switch, with_taps = run
    x, x1, ref, rtaps = bt.case(H, B, T, L)
    d32 = bt.aten_fp32_distance(H, B, T, L)
    geom = bt.geometry(H)
    if switch:                          # read once at mdd_create: the handle below is this run's own
        monkeypatch.setenv(*SWITCH[switch])
    m = _hip().HipModel(geom, bt.state_dict(H), precision=precision, taps=with_taps)
    if switch:
        monkeypatch.delenv(SWITCH[switch][0])
    try:
        xd, x1d = _cuda(x), _cuda(x1)
        _assert_path(m, run, xd, x1d)
        out = torch.empty((T // 2, B, geom.num_class), dtype=torch.float32, device="cuda")
        logp = m.forward(xd, x1d, out=out, sync_errors=True).cpu().numpy()
        errs = {}
        for k in bt.tap_names(geom) if with_taps else []:
            got = m.tap(k).cpu().numpy().astype(np.float64)
            assert got.size == rtaps[k].size, (run, k, got.size, rtaps[k].shape)
            errs[k] = float(np.abs(got.reshape(rtaps[k].shape) - rtaps[k]).max())
        again = m.forward(xd, x1d, out=out, sync_errors=True).cpu().numpy()      # a replay of the graph the first call captured
    finally:
        m.close()
    errs["logp"] = float(np.abs(logp.astype(np.float64) - ref).max())
    tag = _id(run).replace("-", "_")
    tight = [k for k in errs if k == "logp" or k.startswith("rnn")] if precision in ("f32", "f32x6") else []
    ratios = {k: errs[k] / max(d32[k], FLOOR / RATIO) for k in tight}
    print("tiles_" + tag, " ".join("%s %.2e" % kv for kv in errs.items()), "| ratio to ATen fp32:", " ".join("%s %.2f" % kv for kv in ratios.items()))
    for k, e in errs.items():
        record_margin("tiles_%s_%s" % (tag, k), e, TOL)
    for k, r in ratios.items():
        record_margin("tiles_ratio_%s_%s" % (tag, k), r, RATIO)
    for k, e in errs.items():                  # in forward order: the first stage past the bound is the one named
        assert e <= TOL, (run, k, e, errs)
        if k in tight:
            assert e <= max(RATIO * d32[k], FLOOR), (run, k, e, d32[k], errs)
    assert float(np.abs(np.exp(logp.astype(np.float64)).sum(-1) - 1).max()) < 1e-5
    np.testing.assert_array_equal(logp, again)
