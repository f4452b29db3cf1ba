"""The tile walk of gemm_f32x6_kernel on the device (csrc/gemm_raster.h): the walk decides which workgroup computes which tile and when,
never what a C element is -- each keeps its own K order -- so the default walk and MDD_GEMM_X6_RASTER=rows must give the same bits, at
shapes that reach every edge of the block walk and of the launcher's fallback, and the forward must not notice the switch.  What each
shape reaches is pinned, from gemm_raster.h itself, by tests/test_gemm_raster_host.py::test_what_the_device_shapes_reach."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ctc_attention_mispronunciation_amd import synth

pytestmark = pytest.mark.gpu

# M x N x K: what of the walk the shape reaches (192 x 128 tiles, blocks of 4 row panels x 8 column tiles, 8 XCDs x 32 workgroups)
SHAPES = [
    (6912, 1024, 32),     # 36 x 8 = 288 tiles in whole blocks, one K-tile, two rounds
    (7877, 1152, 64),     # 42 panels, the last 5 rows high, x 9 column tiles: 22 blocks would take 3 rounds against 2, so the row walk, two rounds
    (7680, 1000, 96),     # the last column tile partial
    (50000, 3072, 96),    # 24 column tiles, 25 rounds; the last row of blocks one panel high (24 workgroups of each of three XCDs sit the last round out)
    (1728, 3072, 64),     # 9 panels x 24: one round in rows, two in blocks -- the fallback
    (44, 3072, 512),      # the text table's launch: one round, fewer tiles than one XCD's round
    (100, 64, 64),        # tiny launches
    (1, 4, 32),
    (3072, 1920, 64),     # 16 x 15 tiles in one round of blocks: column blocks 8 and 7 wide, and 16 workgroups with no tile at all (the early return)
    (4224, 1536, 64),     # 22 panels x 12 (a training product's shape): 8- and 4-wide blocks in both rounds, the last row of blocks 2 panels high, 64 idle workgroups
    (6100, 2560, 64),     # 32 panels (the last partial) x 20: blocks 8, 8, 4 wide over 3 rounds -- an XCD meets its narrow block in the first, the
                          # middle or the last round, so 80 workgroups sit a round out and take a tile in a later one (tile_of's loop)
]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _x6(A, W, raster, monkeypatch):
    from ctc_attention_mispronunciation_amd import _lib
    L = _lib.lib()
    L.mdd_diag_gemm.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    if raster:
        monkeypatch.setenv("MDD_GEMM_X6_RASTER", raster)
    else:
        monkeypatch.delenv("MDD_GEMM_X6_RASTER", raising=False)
    M, K = A.shape
    N = W.shape[0]
    Cd = torch.full((M, N), float("nan"), device="cuda")
    assert L.mdd_diag_gemm(3, A.data_ptr(), W.data_ptr(), Cd.data_ptr(), M, N, K, None) == 0, L.mdd_last_error().decode()
    torch.cuda.synchronize()
    return Cd


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_walks_give_the_same_bits(M, N, K, monkeypatch):
    """mdd_diag_gemm mode 3 on seeded operands (test_gemm_f32x6_accuracy's: post-ReLU-like A with every seventh column 30 x larger, small
    uniform W): the default walk and the row walk agree in every bit of C, and each is as close to the float64 product as that test asks
    of f32x6 -- mean error at most ATen's fp32 GEMM's, largest error at most 1.5 x ATen's, relative to rms(C)."""
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    rng = np.random.default_rng(K + M)
    A = rng.standard_normal((M, K)).astype(np.float32)
    A[A < 0] = 0.0
    A[:, ::7] *= 30.0
    W = (rng.uniform(-1, 1, (N, K)) * 0.05).astype(np.float32)
    At, Wt = torch.from_numpy(A), torch.from_numpy(W)
    ref = At.double() @ Wt.double().T
    aten = ((At @ Wt.T).double() - ref).abs()
    scale = float(ref.pow(2).mean().sqrt())
    Ad, Wd = At.cuda(), Wt.cuda()
    dflt = _x6(Ad, Wd, None, monkeypatch)
    rows = _x6(Ad, Wd, "rows", monkeypatch)
    assert torch.equal(dflt.view(torch.int32), rows.view(torch.int32)), \
        "%d words differ between the walks" % int((dflt.view(torch.int32) != rows.view(torch.int32)).sum())
    err = (dflt.cpu().double() - ref).abs()     # (rows holds the same bits)
    assert bool(torch.isfinite(err).all())
    got = (float(err.max()) / scale, float(err.mean()) / scale)
    want = (float(aten.max()) / scale, float(aten.mean()) / scale)
    print("GEMM %dx%dx%d |C - C64| / rms(C64), max and mean: f32x6 %.2e %.2e; aten_f32 %.2e %.2e" % (M, N, K, got[0], got[1], want[0], want[1]))
    assert got[1] <= want[1] and got[0] <= 1.5 * want[0]


def test_diag_entries_refuse_a_mistyped_walk(monkeypatch):
    """The mdd_diag_gemm* entries take MDD_GEMM_X6_RASTER per call, for A/B runs: a value that is neither rows nor <rb>x<cb> is MDD_ERR_ARG with a
    message naming it, before anything is launched -- not the default walk under another name."""
    from ctc_attention_mispronunciation_amd import _lib
    L = _lib.lib()
    L.mdd_diag_gemm.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.mdd_diag_gemm_clock.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    A, W, Cd = torch.zeros((4, 32), device="cuda"), torch.zeros((4, 32), device="cuda"), torch.zeros((4, 4), device="cuda")
    ms, mhz = C.c_float(0), C.c_float(0)
    for bad in ("row", "ROWS", "8x8", "4x"):
        monkeypatch.setenv("MDD_GEMM_X6_RASTER", bad)
        assert L.mdd_diag_gemm(3, A.data_ptr(), W.data_ptr(), Cd.data_ptr(), 4, 4, 32, None) == -1
        assert ("mdd_diag_gemm: MDD_GEMM_X6_RASTER=" + bad) in L.mdd_last_error().decode()
        assert L.mdd_diag_gemm_clock(4, 4, 32, 1, C.byref(ms), C.byref(mhz)) == -1
        assert ("mdd_diag_gemm_clock: MDD_GEMM_X6_RASTER=" + bad) in L.mdd_last_error().decode()


def test_forward_does_not_notice_the_switch(monkeypatch):
    """A fused f32x6 forward of two batches of different lengths, through three graph replays, under the default walk and under
    MDD_GEMM_X6_RASTER=rows (read at create): the same log-prob bits.  At this size every projection takes the row walk either way; the case
    pins that the switch's way into the handle leaves the forward alone."""
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    geom = synth.Geometry(**synth.REFERENCE)
    sd = synth.synth_state_dict(geom, seed=1234)
    shapes = [(5, 120, 9), (3, 64, 4)]
    Bt, Tm, Lm = sum(s[0] for s in shapes), max(s[1] for s in shapes), max(s[2] for s in shapes)
    X = np.zeros((Bt, Tm, geom.feat), dtype=np.float32)
    X1 = np.zeros((Bt, Lm), dtype=np.int64)
    frames, canon = np.zeros(Bt, dtype=np.int32), np.zeros(Bt, dtype=np.int32)
    r = 0
    for k, (b, T, L) in enumerate(shapes):
        x, x1, _, _ = synth.synth_batch(geom, B=b, T=T, L=L, seed=7 + 31 * k, ragged=True)
        X[r:r + b, :T] = x; X1[r:r + b, :L] = x1; frames[r:r + b] = T // 2; canon[r:r + b] = L
        r += b
    runs = {}
    for raster in (None, "rows"):
        if raster:
            monkeypatch.setenv("MDD_GEMM_X6_RASTER", raster)
        else:
            monkeypatch.delenv("MDD_GEMM_X6_RASTER", raising=False)
        m = HipModel(geom, sd, precision="f32x6")
        assert m.precision == "f32x6"
        runs[raster] = [m.forward_fused(_cuda(X), _cuda(X1), _cuda(frames), _cuda(canon), sync_errors=True).cpu().numpy() for _ in range(4)]
    for raster, outs in runs.items():
        for again in outs[1:]:          # the replays of the graph the first call captured: every defined row
            for b in range(Bt):
                np.testing.assert_array_equal(again[:frames[b], b].view(np.int32), outs[0][:frames[b], b].view(np.int32))
    for b in range(Bt):
        np.testing.assert_array_equal(runs[None][0][:frames[b], b].view(np.int32), runs["rows"][0][:frames[b], b].view(np.int32))
