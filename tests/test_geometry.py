"""The decode forward across the plan space (GPU): every geometry of tests/geometry_cases.py::DECODE -- unfused conv into the fast GEMMs,
1..6 layers, unpacked hidden sizes, 2..101 classes on both attention tails, embedding tables of 1..100 rows x 32..512 -- in every
requested precision against oracle/ref_port.forward in float64: log-probs and every tap, on the two ragged batches the other modules
use.  Each row also asserts the kernels csrc/plan.h is expected to give it (HipModel.precision, the stage list of HipModel.profile), so
a change of the policy fails a test instead of silently changing what these tests cover.

The bound is the project's 1e-4 on log-probs and taps for every geometry and mode; the reference side stays under 1e-5
(tests/test_geometry_reference.py).  Every measured distance is recorded under a key starting "geom_" (tests.helpers.record_margin);
the GPU run's values are committed as profiles/geometry_margins.json."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import geometry_cases as gc
from tests.helpers import record_margin
from ctc_attention_mispronunciation_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-4
MDD_ERR_ARG = -1


def _hip():
    from ctc_attention_mispronunciation_amd import hip_model
    return hip_model


def _lib():
    from ctc_attention_mispronunciation_amd import _lib
    return _lib


def _cuda(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()      # (the cached cases are read-only)


@functools.lru_cache(maxsize=None)
def _sd(name):
    return synth.synth_state_dict(gc.decode_geometry(name), seed=1234)


@functools.lru_cache(maxsize=None)
def _case(name, B, T, L, seed):
    """(x, x1, float64 log-probs, float64 taps with "score"): computed once per geometry and shape, shared by the three precisions."""
    from oracle import ref_port
    torch.set_num_threads(min(16, torch.get_num_threads()))
    geom = gc.decode_geometry(name)
    x, x1 = gc.draw_batch(geom, B, T, L, seed)
    assert x1.max() == geom.emb_rows - 1
    taps = {}
    logp = ref_port.forward(_sd(name), x, x1, dtype=torch.float64, taps=taps).numpy()
    assert logp.dtype == np.float64
    taps["score"] = gc.reference_scores(taps, geom.layers)
    for a in [x, x1, logp] + list(taps.values()):
        a.setflags(write=False)
    return x, x1, logp, taps


class _Handle(object):
    def __init__(self, name, precision):
        self.m = _hip().HipModel(gc.decode_geometry(name), _sd(name), precision=precision, taps=True)

    def __enter__(self):
        return self.m

    def __exit__(self, *exc):
        self.m.close()


def _assert_plan(m, name, requested, x, x1):
    """The observables of plan_forward's choice: the precision in effect and the stage list with its launch counts."""
    geom = m.geom
    want_prec, want_conv, want_lstm = (gc.DECODE.get(name) or gc.DECODE_LIMIT_EXTRA[name])[1][requested]
    assert m.precision == want_prec, (name, requested, m.precision)
    prof = m.profile(_cuda(x), _cuda(x1))
    launches = {n: l for n, _, l, _ in prof}
    names = [n for n, _, _, _ in prof]
    if want_conv == "fused":
        assert "conv_fused" in names and "conv0" not in names and "conv1" not in names, names
    else:
        assert "conv0" in names and "conv1" in names and "conv_fused" not in names, names
    Tp, L = x.shape[1] // 2, x1.shape[1]
    for n in range(geom.layers):
        assert launches["lstm%d" % n] == (1 if want_lstm == "layer" else Tp), (name, requested, n, launches)
    assert launches["lstm_text"] == (1 if want_lstm == "layer" else L), (name, requested, launches)
    assert names.count("gemm_ih0") == 1 and "lstm%d" % geom.layers not in names


def _compare(m, name, requested, shape, seed):
    B, T, L = shape
    x, x1, ref, rtaps = _case(name, B, T, L, seed)
    geom = m.geom
    xd, x1d = _cuda(x), _cuda(x1)
    out = torch.empty((T // 2, B, geom.num_class), dtype=torch.float32, device="cuda")
    logp = m.forward(xd, x1d, out=out, sync_errors=True).cpu().numpy()
    tag = "geom_%s_%s_B%d" % (name, requested, B)
    errs = {}
    for k in ["conv1"] + ["rnn%d" % i for i in range(geom.layers)] + ["text", "key", "score"]:
        got = m.tap(k).cpu().numpy().astype(np.float64)
        assert got.size == rtaps[k].size, (tag, k, got.size, rtaps[k].shape)
        errs[k] = float(np.abs(got.reshape(rtaps[k].shape) - rtaps[k]).max())
    again = m.forward(xd, x1d, out=out, sync_errors=True).cpu().numpy()      # a replay of the graph the first call captured
    errs["logp"] = float(np.abs(logp.astype(np.float64) - ref).max())
    print(tag, " ".join("%s %.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        record_margin("%s_%s" % (tag, k), e, TOL)
    for k, e in errs.items():                  # in forward order: the first stage past the bound is the one named
        assert e <= TOL, (tag, k, e, errs)
    assert float(np.abs(np.exp(logp.astype(np.float64)).sum(-1) - 1).max()) < 1e-5
    np.testing.assert_array_equal(logp, again)


@pytest.mark.parametrize("precision", gc.PRECISIONS)
@pytest.mark.parametrize("name", sorted(gc.DECODE))
def test_forward_parity_and_plan(name, precision):
    with _Handle(name, precision) as m:
        x, x1, _, _ = _case(name, *gc.SMALL, 5)
        _assert_plan(m, name, precision, x, x1)
        _compare(m, name, precision, gc.SMALL, 5)
        _compare(m, name, precision, gc.WIDE, 65)


# ------------------------------------------------------------------------------------------- the other entry points
@pytest.mark.parametrize("precision", gc.PRECISIONS)
@pytest.mark.parametrize("name", gc.MID)
@pytest.mark.parametrize("T_raw", [23, 8])
def test_forward_raw_equals_stack_then_forward(name, precision, T_raw):
    """mdd_forward_raw gives the bits of stack_features followed by forward: through the fused front end's index map (H 128 and H 256 /
    C 49 in mode 2, the latter in mode 1 too) and through the stacked copy in front of conv0 (feat 120; every geometry in mode 0).
    T_raw = 23: the repeated last frame and the zero row that pads to an even count."""
    from ctc_attention_mispronunciation_amd.utils.data_loader import stack_features
    geom = gc.decode_geometry(name)
    raw = _cuda(synth.synth_raw_features(3, T_raw, geom.feat // 3, seed=T_raw))
    _, x1 = gc.draw_batch(geom, 3, 2, 5, seed=1)
    x1 = _cuda(x1)
    with _Handle(name, precision) as m:
        assert m.precision == gc.DECODE[name][1][precision][0]
        want = m.forward(stack_features(raw), x1, sync_errors=True).cpu().numpy()
        got = m.forward_raw(raw, x1, sync_errors=True).cpu().numpy()
    assert want.shape == (_lib().lib().mdd_stack_len(T_raw, 2, 2) // 2, 3, geom.num_class)
    np.testing.assert_array_equal(got, want)


FUSED_SHAPES = [(3, 12, 5), (2, 20, 70), (4, 8, 64)]      # (b, T_g, L_g): three batches, L on both sides of 64


@pytest.mark.parametrize("precision", gc.PRECISIONS)
@pytest.mark.parametrize("name", gc.MID)
def test_fused_batches_equal_their_own_runs(name, precision):
    """mdd_forward_fused over three batches of different (T, L): every utterance's defined rows bit-identical to mdd_forward on its batch
    alone, through the per-step recurrences (H 128: seqlen holds the reverse direction back), both attention tails and the layer kernels."""
    geom = gc.decode_geometry(name)
    batches = [gc.draw_batch(geom, b, T, L, seed=7 + 31 * k) for k, (b, T, L) in enumerate(FUSED_SHAPES)]
    Bt, Tm, Lm = sum(s[0] for s in FUSED_SHAPES), max(s[1] for s in FUSED_SHAPES), max(s[2] for s in FUSED_SHAPES)
    X = np.zeros((Bt, Tm, geom.feat), dtype=np.float32)
    X1 = np.zeros((Bt, Lm), dtype=np.int64)
    frames, canon = np.zeros(Bt, dtype=np.int32), np.zeros(Bt, dtype=np.int32)
    r = 0
    for (x, x1), (b, T, L) in zip(batches, FUSED_SHAPES):
        X[r:r + b, :T] = x; X1[r:r + b, :L] = x1; frames[r:r + b] = T // 2; canon[r:r + b] = L
        r += b
    with _Handle(name, precision) as m:
        alone = [m.forward(_cuda(x), _cuda(x1), sync_errors=True).cpu().numpy() for x, x1 in batches]
        fused = m.forward_fused(_cuda(X), _cuda(X1), _cuda(frames), _cuda(canon), sync_errors=True).cpu().numpy()
    r = 0
    for lp, (b, T, L) in zip(alone, FUSED_SHAPES):
        assert np.isfinite(lp).all()
        np.testing.assert_array_equal(fused[:T // 2, r:r + b], lp, err_msg="batch with (T, L) = (%d, %d)" % (T, L))
        r += b


# ------------------------------------------------------------------------------------------- the canonical-length limit
@pytest.mark.parametrize("name", sorted(gc.LIMIT))
def test_canonical_length_limit_away_from_the_reference_widths(name):
    """include/mdd_hip.h at mdd_forward: L <= 2364 - 2H with the matrix-core tail (H 128 / C 45: 2108), L <= 2560 - 4H - C with the
    scalar tail (H 128 / C 49: 1999).  At the limit the forward is within 1e-4 of float64; one phoneme more returns MDD_ERR_ARG naming L,
    leaves logp untouched and the handle usable (the same bits for the limit case afterwards)."""
    lib = _lib().lib()
    geom = gc.decode_geometry(name)
    L = gc.LIMIT[name]
    x, x1, ref, _ = _case(name, 1, 4, L, L)
    xd, x1d = _cuda(x), _cuda(x1)
    xl, x1l = gc.draw_batch(geom, 1, 4, L + 1, seed=L + 1)
    xld, x1ld = _cuda(xl), _cuda(x1l)
    with _Handle(name, "f32x6") as m:
        assert m.precision == "f32x6"
        logp = m.forward(xd, x1d, sync_errors=True).cpu().numpy()
        err = float(np.abs(logp.astype(np.float64) - ref).max())
        print("geom_limit_%s_L%d: max|logp - ref64| = %.3e" % (name, L, err))
        record_margin("geom_limit_%s_L%d_logp" % (name, L), err, TOL)
        assert err <= TOL, (name, L, err)
        out = torch.full((2, 1, geom.num_class), 12345.0, dtype=torch.float32, device="cuda")
        st = _lib().current_stream_ptr()
        rc = lib.mdd_forward(m.handle, C.c_void_p(xld.data_ptr()), 1, 4, C.c_void_p(x1ld.data_ptr()), L + 1, C.c_void_p(out.data_ptr()), st)
        assert rc == MDD_ERR_ARG
        assert ("L=%d" % (L + 1)) in lib.mdd_last_error().decode()
        assert lib.mdd_sync(m.handle, st) == 0
        torch.cuda.synchronize()
        assert bool((out == 12345.0).all())
        after = m.forward(xd, x1d, sync_errors=True).cpu().numpy()
    np.testing.assert_array_equal(after, logp)
