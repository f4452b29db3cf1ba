"""The 256 x 128 tile of gemm_f32x6_kernel (four 16-row MFMA tiles per wave, RT = 4; csrc/gemm_bf16x6.hip) against the 192 x 128 one
(RT = 3).  RT = 4 keeps a lane's hi.hi total `tot` in LDS behind the two W stages instead of in registers; the arithmetic of a C element
is RT = 3's -- tot = 0 at the tile's start, tot = tot + hh at each segment's end, (tot + sm) + bias at the end -- so MDD_GEMM_X6_RT=4 and =3
must give the same bits: at shapes that reach every count of K-tiles and segments, the panel edge, and a workgroup's second tile; and
a forward must not notice which tile its projections and its text table were multiplied on."""
import ctypes as C

import numpy as np
import pytest
import torch

from ctc_attention_mispronunciation_amd import synth

pytestmark = pytest.mark.gpu

# M x N x K, raster: what of the RT = 4 kernel the shape reaches (K-tile 32, segments of 8 K-tiles, K-tiles taken in pairs)
SHAPES = [
    (1, 4, 32, None),          # one K-tile
    (255, 128, 256, None),     # the panel edge from below: one whole segment
    (256, 128, 256, None),     # a whole panel
    (257, 132, 288, None),     # a second panel of one row, a column tail, one whole segment plus one K-tile
    (64, 128, 64, None),       # a pair of K-tiles
    (64, 128, 96, None),       # an odd count of K-tiles
    (64, 128, 544, None),      # two segments and a remainder (17 K-tiles)
    (64, 128, 1952, None),     # 61 K-tiles: the eighth segment, 5 K-tiles long
    (768, 12800, 64, None),    # 300 tiles on 256 workgroups: a workgroup's second tile must start from a zeroed `tot`
    (768, 12800, 64, "rows"),  # the same in the row walk
]


def _x6(A, W, rt, raster, monkeypatch):
    from ctc_attention_mispronunciation_amd import _lib
    L = _lib.lib()
    L.mdd_diag_gemm.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    monkeypatch.setenv("MDD_GEMM_X6_RT", rt)
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


@pytest.mark.parametrize("M,N,K,raster", SHAPES)
def test_rt4_gives_rt3_s_bits(M, N, K, raster, monkeypatch):
    """mdd_diag_gemm mode 3 on seeded operands (tests/test_gemm_raster.py's kind: post-ReLU-like A with every seventh column 30 x larger,
    small uniform W; here also an all-zero A row and an all-zero W row, whose C entries are +0 only if `tot` starts from +0 and receives
    hh in the order tot + hh): MDD_GEMM_X6_RT=4 and =3 agree in every bit of C, and nothing is left unwritten."""
    rng = np.random.default_rng(K + M)
    A = rng.standard_normal((M, K)).astype(np.float32)
    A[A < 0] = 0.0
    A[:, ::7] *= 30.0
    A[M // 2] = 0.0
    W = (rng.uniform(-1, 1, (N, K)) * 0.05).astype(np.float32)
    W[N // 3] = 0.0
    Ad, Wd = torch.from_numpy(A).cuda(), torch.from_numpy(W).cuda()
    c3 = _x6(Ad, Wd, "3", raster, monkeypatch)
    c4 = _x6(Ad, Wd, "4", raster, monkeypatch)
    assert bool(torch.isfinite(c3).all()) and bool(torch.isfinite(c4).all())
    b3, b4 = c3.view(torch.int32), c4.view(torch.int32)
    assert torch.equal(b4, b3), "%d words differ between RT = 4 and RT = 3" % int((b4 != b3).sum())
    assert bool((b4[M // 2] == 0).all()) and bool((b4[:, N // 3] == 0).all())     # +0, not -0


def test_diag_entries_refuse_a_mistyped_tile(monkeypatch):
    """The mdd_diag_gemm* entries take MDD_GEMM_X6_RT per call: a value that is neither 3 nor 4 is MDD_ERR_ARG with a message naming it,
    before anything is launched."""
    from ctc_attention_mispronunciation_amd import _lib
    L = _lib.lib()
    L.mdd_diag_gemm.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.mdd_diag_gemm_clock.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.mdd_diag_gemm_time.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
    A, W, Cd = torch.zeros((4, 32), device="cuda"), torch.zeros((4, 32), device="cuda"), torch.zeros((4, 4), device="cuda")
    ms, mhz = C.c_float(0), C.c_float(0)
    monkeypatch.delenv("MDD_GEMM_X6_RASTER", raising=False)
    for bad in ("2", "5", "34", "4 ", "four", ""):
        monkeypatch.setenv("MDD_GEMM_X6_RT", bad)
        assert L.mdd_diag_gemm(3, A.data_ptr(), W.data_ptr(), Cd.data_ptr(), 4, 4, 32, None) == -1
        assert ("mdd_diag_gemm: MDD_GEMM_X6_RT=" + bad) in L.mdd_last_error().decode()
        assert L.mdd_diag_gemm_clock(4, 4, 32, 1, C.byref(ms), C.byref(mhz)) == -1
        assert ("mdd_diag_gemm_clock: MDD_GEMM_X6_RT=" + bad) in L.mdd_last_error().decode()
        assert L.mdd_diag_gemm_time(3, 4, 4, 32, 1, C.byref(ms)) == -1
        assert ("mdd_diag_gemm_time: MDD_GEMM_X6_RT=" + bad) in L.mdd_last_error().decode()
        assert L.mdd_diag_gemm_ops(3, 0, 0, A.data_ptr(), 32, W.data_ptr(), 32, Cd.data_ptr(), 4, 4, 4, 32, 1, None) == -1
        assert ("mdd_diag_gemm_ops: MDD_GEMM_X6_RT=" + bad) in L.mdd_last_error().decode()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_forward_does_not_notice_the_tile(monkeypatch):
    """A model whose projections have more than 256 rows (B = 3 at T = 200: 300 rows, two panels either way; H = 384), built with the
    default (the rule of csrc/gemm_raster.h per launch), with MDD_GEMM_X6_RT=3 and with =4 at create (=4 also passes the biased text
    table's 44-row product through the 256-row tile): the same log-prob bits and the same bits in every layer tap, through three graph
    replays, and again after a second finalize on the same handle."""
    from ctc_attention_mispronunciation_amd.hip_model import HipModel
    geom = synth.Geometry(**synth.REFERENCE)
    assert geom.hidden == 384
    sd = synth.synth_state_dict(geom, seed=1234)
    sd2 = synth.synth_state_dict(geom, seed=77)
    B, T, L = 3, 200, 9
    x, x1, _, _ = synth.synth_batch(geom, B=B, T=T, L=L, seed=11, ragged=False)
    taps = ["rnn%d" % i for i in range(geom.layers)] + ["text", "key"]
    monkeypatch.delenv("MDD_GEMM_X6_RASTER", raising=False)
    runs = {}
    for rt in (None, "3", "4"):
        if rt:
            monkeypatch.setenv("MDD_GEMM_X6_RT", rt)
        else:
            monkeypatch.delenv("MDD_GEMM_X6_RT", raising=False)
        m = HipModel(geom, sd, taps=True, precision="f32x6")
        assert m.precision == "f32x6"
        got = []
        for weights in (None, sd2):
            if weights is not None:
                m.load_state_dict(weights)      # a second finalize on the same handle: the text table is multiplied again
            outs = [m.forward(_cuda(x), _cuda(x1), sync_errors=True).clone() for _ in range(4)]
            for again in outs[1:]:              # the replays of the graph the first call captured
                assert torch.equal(again.view(torch.int32), outs[0].view(torch.int32))
            got.append([outs[0]] + [m.tap(t).clone() for t in taps])
        runs[rt] = got
        m.close()
    assert runs[None][0][1].numel() == (T // 2) * B * 2 * geom.hidden == 300 * 768
    assert not torch.equal(runs["3"][0][0], runs["3"][1][0])      # the second weight set is another model
    for rt in (None, "4"):
        for k in range(2):
            for what, g, w in zip(["logp"] + taps, runs[rt][k], runs["3"][k]):
                assert g.shape == w.shape and torch.equal(g.view(torch.int32), w.view(torch.int32)), (rt, k, what)
