"""The HIP fbank kernels (fbank_kernel / fbank_batch_kernel, csrc/fbank.hip) against the float64 restatement of
tests/fbank_reference.py, element by element, under its conditioning model: every output within max(1, 4 * k32) model units, where
k32 is what a plain float32 numpy implementation needs on the same case (at most 4: tests/test_fbank_reference.py).  No element is
masked; the floor is inside the model.  The batched kernel and its stacking are held to float64 rows moved by oracle.stack_skip,
not to the per-utterance kernel."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import fbank_reference as R
from tests.helpers import GOLD, record_margin

pytestmark = pytest.mark.gpu

CASE_NAMES = list(R.CASES)
BATCH_NAMES = [n for n in CASE_NAMES if R.CASES[n].size >= R.N]
SMALL_BATCH = ["length_400", "length_560", "length_1040", "noise_3000"]          # 400, 560, 1040 and 4000 samples
FLOOR_ULP = float(np.spacing(np.float32(abs(R.LOG_FLOOR))))


def _fb():
    from ctc_attention_mispronunciation_amd.utils import fbank as fb
    return fb


def _cmvn():
    fb = _fb()
    scale, offset = fb.cmvn_scale_offset(fb.read_cmvn_stats(os.path.join(GOLD, "global_fbank_cmvn.txt")))
    assert scale.dtype == offset.dtype == np.float32 and scale.shape == offset.shape == (R.COLS,)
    return scale, offset


def _want(name, cmvn):
    """(float64 rows [T, 81], their limit in model units) of a case, without or with CMVN."""
    r, lim, _ = R.reference(name)
    if cmvn is None:
        return r.logs, lim
    return R.cmvn64(r.logs, *cmvn), R.cmvn_limit(r.logs, lim, *cmvn)


def _measure(got, want, lim):
    """(largest |got - want| / limit in model units, largest |got - want|); an output that is not finite measures as inf."""
    if not want.size:
        return 0.0, 0.0
    dist = np.abs(got.astype(np.float64) - want)
    dist = np.where(np.isfinite(dist), dist, np.inf)
    return float((dist / lim).max()), float(dist.max())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fbank_kernel_within_the_model_of_float64(name):
    fb = _fb()
    from ctc_attention_mispronunciation_amd import _lib
    x = R.CASES[name]
    k32, k = R.reference(name)[2], R.gpu_k(name)
    frames = _lib.lib().mdd_fbank_num_frames(x.size)
    assert frames == R.num_frames(x.size)
    failures = []
    for tag, cmvn in (("", None), ("_cmvn", _cmvn())):
        want, lim = _want(name, cmvn)
        got = fb.compute_fbank_feats(x, cmvn=cmvn).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape == (frames, R.COLS)
        units, dist = _measure(got, want, lim)
        print("%s%s: %.3f model units (limit %.2f, plain float32 %.3f), largest distance %.2e" % (name, tag, units, k, k32, dist))
        record_margin("fbank_%s%s" % (name, tag), units, k)
        record_margin("fbank_%s%s_abs" % (name, tag), dist)
        if not units <= k:
            failures.append((tag, units, k, dist))
        if cmvn is None:
            record_margin("fbank_%s_k32" % name, k32, 4.0)
            if name in R.FLOOR_CASES:
                assert np.abs(got.astype(np.float64) - R.LOG_FLOOR).max() <= FLOOR_ULP
    assert not failures, failures


def _stack_sources(T, right, skip, n_down):
    """[T_out, right + 1] raw frame index behind every stacked slot, -1 for a padding row: oracle.stack_skip run on the frame
    numbers themselves, so the float64 rows keep their precision while the index arithmetic stays the oracle's."""
    src = oracle.stack_skip(np.arange(1, T + 1, dtype=np.float32)[:, None], right=right, skip=skip, n_down=n_down)
    assert src.shape[1] == right + 1
    return src.astype(np.int64) - 1


def _check_batch(names, cmvn, right, skip, n_down, tag):
    fb = _fb()
    wavs = [R.CASES[n] for n in names]
    srcs = [_stack_sources(R.num_frames(w.size), right, skip, n_down) for w in wavs]
    t_out = max(s.shape[0] for s in srcs)
    W = (right + 1) * R.COLS
    out = torch.full((len(wavs), t_out, W), float("nan"), dtype=torch.float32, device="cuda")
    x, sizes = fb.fbank_batch(wavs, cmvn=cmvn, right_ctx=right, n_skip_frame=skip, n_downsample=n_down, out=out)
    assert x.data_ptr() == out.data_ptr() and tuple(x.shape) == (len(wavs), t_out, W)
    got = x.cpu().numpy()
    want_sizes = np.array([np.float32(s.shape[0] / t_out) for s in srcs], dtype=np.float32)
    assert sizes.dtype == torch.float32 and np.array_equal(sizes.numpy(), want_sizes)
    assert np.isfinite(got).all()                                   # every element written, padding included
    failures, worst = [], 0.0
    for b, (name, src) in enumerate(zip(names, srcs)):
        rows, lim = _want(name, cmvn)
        pad = np.repeat(src < 0, R.COLS, axis=1)                    # [T_b, W]
        want = np.where(pad, 0.0, rows[np.maximum(src, 0)].reshape(src.shape[0], W))
        wlim = np.where(pad, 0.0, lim[np.maximum(src, 0)].reshape(src.shape[0], W))
        mine = got[b, :src.shape[0]].astype(np.float64)
        assert not got[b, src.shape[0]:].any() and not mine[pad].any(), name          # batch padding and even-pad rows: zero
        dist = np.abs(mine - want)
        units = float((dist[~pad] / wlim[~pad]).max())
        worst = max(worst, units / R.gpu_k(name))
        if not np.all(dist <= R.gpu_k(name) * wlim):
            failures.append((name, units, R.gpu_k(name), float(dist.max())))
    print("%s: B %d, T_out %d, worst case at %.3f of its limit" % (tag, len(wavs), t_out, worst))
    record_margin("fbank_batch_%s" % tag, worst, 1.0)
    assert not failures, failures
    return wavs, x


@pytest.mark.parametrize("use_cmvn", [False, True])
def test_fbank_batch_kernel_within_the_model_of_float64(use_cmvn):
    """Every case of at least one window as one ragged batch with the shipped right_ctx = 2, n_skip_frame = 2, n_downsample = 2."""
    _check_batch(BATCH_NAMES, _cmvn() if use_cmvn else None, 2, 2, 2, "all_r2_s2_d2" + ("_cmvn" if use_cmvn else ""))


@pytest.mark.parametrize("right,skip,n_down", [(0, 1, 1), (3, 3, 2)])
def test_fbank_batch_stacking_geometries_against_float64(right, skip, n_down):
    """1, 2, 5 and 23 raw frames: no context and no skip; and a context that outruns the skip, where the last frame repeats
    across both `right` and `skip` and an even-pad row follows."""
    _check_batch(SMALL_BATCH, _cmvn(), right, skip, n_down, "small_r%d_s%d_d%d" % (right, skip, n_down))


def test_fbank_batch_device_offsets_give_the_list_forms_bits():
    fb = _fb()
    cmvn = _cmvn()
    wavs = [R.CASES[n] for n in BATCH_NAMES]
    x, sizes = fb.fbank_batch(wavs, cmvn=cmvn)
    offsets = np.concatenate([[0], np.cumsum([w.size for w in wavs])]).astype(np.int64)
    dev = torch.from_numpy(np.concatenate(wavs)).cuda()
    x2, sizes2 = fb.fbank_batch(dev, cmvn=cmvn, offsets=offsets)
    assert torch.equal(x, x2) and torch.equal(sizes, sizes2)
    x3, _ = fb.fbank_batch(dev, cmvn=cmvn, offsets=torch.from_numpy(offsets))
    assert torch.equal(x, x3)


def test_fbank_kernels_are_deterministic():
    fb = _fb()
    cmvn = _cmvn()
    for name in ("word_1", "tone_7900Hz_noise_3", "dc_-30000_noise_3", "length_1040"):
        a = fb.compute_fbank_feats(R.CASES[name], cmvn=cmvn)
        b = fb.compute_fbank_feats(R.CASES[name], cmvn=cmvn)
        assert a.numel() and torch.equal(a, b), name
    wavs = [R.CASES[n] for n in SMALL_BATCH]
    assert torch.equal(fb.fbank_batch(wavs, cmvn=cmvn)[0], fb.fbank_batch(wavs, cmvn=cmvn)[0])
