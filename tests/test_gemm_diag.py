"""The GEMM diagnostics after their move to csrc/diag.hip, and the two things that changed under them: launch_split3 runs the padded
three-plane kernel (split3_pad_kernel with Kp == K), and the f32x6 prototype (mode 2 of mdd_diag_gemm) is gone."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests.test_gpu_parity import _cuda

pytestmark = pytest.mark.gpu

MDD_ERR_ARG = -1
PLANE_SHAPES = [(1, 32), (17, 32), (16, 64), (50, 96)]   # (rows, K): a partial 16-row group, one K-tile, several K-tiles


def _lib():
    from ctc_attention_mispronunciation_amd import _lib as L
    lib = L.lib()
    lib.mdd_diag_gemm.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


def _gemm(mode, A, W):
    L = _lib()
    Ad, Wd = _cuda(A), _cuda(W)
    Cd = torch.full((A.shape[0], W.shape[0]), -7.5, device="cuda")
    rc = L.mdd_diag_gemm(mode, Ad.data_ptr(), Wd.data_ptr(), Cd.data_ptr(), A.shape[0], W.shape[0], A.shape[1], None)
    return rc, L.mdd_last_error().decode(), Cd.cpu().numpy()


@pytest.mark.parametrize("rows,K", PLANE_SHAPES)
def test_split3_planes_through_the_padded_kernel(rows, K):
    """mdd_diag_gemm mode 3 splits both operands with launch_split3.  With W the K x K identity every C element is one non-zero product
    per plane pair and hi + mid + lo == x, so C must be A bit for bit: a plane, row, K-tile or chunk taken from the wrong place, or a
    rounding that is not split3's, shows.  Integer operands below 2^24 in every partial sum: C equals numpy's integer product."""
    rng = np.random.default_rng(100 * rows + K)
    A = rng.standard_normal((rows, K)).astype(np.float32)
    rc, err, got = _gemm(3, A, np.eye(K, dtype=np.float32))
    assert rc == 0, err
    np.testing.assert_array_equal(got.view(np.int32), A.view(np.int32))
    Ai = rng.integers(-4095, 4096, (rows, K))          # 12 bits: hi and mid planes both carry part of it
    Wi = rng.integers(-4, 5, (K, K))                   # |sum| <= 4095 * 4 * 96 < 2^21
    rc, err, got = _gemm(3, Ai.astype(np.float32), Wi.astype(np.float32))
    assert rc == 0, err
    np.testing.assert_array_equal(got, (Ai @ Wi.T).astype(np.float32))


def test_retired_prototype_mode_is_refused():
    """mode 2 (the f32x6 prototype through three x3 launches) no longer exists: MDD_ERR_ARG, and the message names the modes that do"""
    rc, err, got = _gemm(2, np.ones((16, 32), np.float32), np.ones((32, 32), np.float32))
    assert rc == MDD_ERR_ARG
    assert {"0", "1", "3"} <= set(re.findall(r"\b\d\b", err.split("(", 1)[1])), err
    assert (got == -7.5).all()


def test_race_screen_entry_reports_times_and_leaves_retired_slots(monkeypatch):
    """mdd_diag_gemm_ph8 with a times array: both kernels' mean times arrive, and the slots of the retired forms ([2] DMA-in-M, [7..10] its
    stamps, [11] A-first, [12] store-less) are not written"""
    monkeypatch.delenv("MDD_GEMM_STAMP", raising=False)
    monkeypatch.delenv("MDD_GEMM_T128", raising=False)
    L = _lib()
    torch.zeros(1).cuda()
    bad, ms = C.c_uint(12345), (C.c_float * 16)(*([-3.0] * 16))
    rc = L.mdd_diag_gemm_ph8(C.c_int(256), C.c_int(512), C.c_int(32), C.c_int(2), C.c_uint(1), C.byref(bad), ms)
    assert rc == 0, L.mdd_last_error().decode()
    assert bad.value == 0
    assert ms[0] > 0 and ms[1] > 0
    assert [ms[i] for i in (2, 7, 8, 9, 10, 11, 12)] == [-3.0] * 7
