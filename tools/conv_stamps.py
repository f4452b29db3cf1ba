"""Diagnostic: time of the f32x6 conv front end alone (default and row-at-a-time kernels), whether the two agree on every output word,
and the stamped phase split of the default kernel per block of two output rows (mdd_diag_conv_time).
usage: conv_stamps.py [B T]...   (default: 512 500, 192 500, 64 500)"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from ctc_attention_mispronunciation_amd import _lib
L = _lib.lib()
torch.zeros(1).cuda()
L.mdd_diag_conv_time.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
PH = ["wait top", "x store", "barrier", "conv0+x req", "barrier", "conv1", "barrier", "epilogue", "barrier", "stores"]
a = [int(v) for v in sys.argv[1:]]
shapes = list(zip(a[0::2], a[1::2])) or [(512, 500), (192, 500), (64, 500)]
for B, T in shapes:
    ms, ms_row, bad = C.c_float(0), C.c_float(0), C.c_longlong(-1)
    ph = (C.c_double * 80)()
    rc = L.mdd_diag_conv_time(B, T, 10, 0, C.byref(ms), ph, C.byref(bad))
    assert rc == 0, L.mdd_last_error().decode()
    rc = L.mdd_diag_conv_time(B, T, 10, 1, C.byref(ms_row), None, None)
    assert rc == 0, L.mdd_last_error().decode()
    print("B = %d, T = %d: default %.4f ms, row-wise %.4f ms, differing output words %d" % (B, T, ms.value, ms_row.value, bad.value))
    S = max(1, min(T // 2, (512 + B - 1) // B))
    seg = ((T // 2 + S - 1) // S + 1) // 2 * 2
    blocks = (seg + 1) // 2                          # blocks of two rows a workgroup with a whole segment walks
    print("  cycles per block of two output rows (%d blocks per workgroup), by wave:" % blocks)
    print("  %-12s" % "phase" + "".join("%8d" % w for w in range(8)))
    for i, name in enumerate(PH):
        print("  %-12s" % name + "".join("%8.0f" % (ph[w * 10 + i] / blocks) for w in range(8)))
    print("  %-12s" % "sum" + "".join("%8.0f" % (sum(ph[w * 10 + i] for i in range(10)) / blocks) for w in range(8)))
