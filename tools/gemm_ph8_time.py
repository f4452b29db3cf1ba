"""Time the projection GEMM's two 256x256 forms on the bench's shapes (single-barrier, 8-phase) and screen them against each other:
python tools/gemm_ph8_time.py   (MDD_GEMM_T128=1: the 128x128 kernel too; MDD_GEMM_STAMP=1: the 8-phase kernel's phase stamps)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401
from ctc_attention_mispronunciation_amd import _lib  # noqa: E402

L = _lib.lib()
torch.zeros(1).cuda()
for M, N, K in ((128000, 3072, 768), (128000, 3072, 1952), (16000, 3072, 768), (20480, 3072, 512)):
    bad, ms = C.c_uint(0), (C.c_float * 16)()
    rc = L.mdd_diag_gemm_ph8(M, N, K, 6, 1, C.byref(bad), ms)
    fl = 2.0 * M * N * K
    print("M=%d N=%d K=%d rc=%d mismatches=%d  single-barrier %.3f ms (%.0f TF)  8-phase %.3f ms (%.0f TF)" %
          (M, N, K, rc, bad.value, ms[0], fl / ms[0] / 1e9, ms[1], fl / ms[1] / 1e9))
    if os.environ.get("MDD_GEMM_T128"):
        print("   128x128 kernel, two workgroups per CU: %.3f ms (%.0f TF)" % (ms[14], fl / ms[14] / 1e9))
    if os.environ.get("MDD_GEMM_STAMP"):
        print("   cycles per K-tile and wave: load bodies %.0f, waiting at their barriers %.0f, MFMA bodies %.0f (floor 4 x 24 x 16 = 1536), waiting at theirs %.0f"
              % (ms[3], ms[4], ms[5], ms[6]))
