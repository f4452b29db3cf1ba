"""Diagnostic: kernel time of the projection GEMM shapes in each arithmetic (mdd_diag_gemm_time), and of the f32x6 kernel under each tile
walk with the clock the chip held inside it (mdd_diag_gemm_clock).

  python tools/gemm_time.py [0] [1] [3]                 one line per shape and arithmetic (0 exact fp32 MFMA, 1 split-bf16 x3, 3 f32x6)
  python tools/gemm_time.py --raster [ARM ...]          f32x6 only: the arms (values of MDD_GEMM_X6_RASTER; default rows 2x16 4x8 8x4) in
        [--cycles N] [--seconds S]                      turn, N times over, each visit S seconds of back-to-back launches (default 5, 2.0)
                                                        on random operands, then the stamped launch: median and min of the visits'
                                                        mean kernel times, and the median in-kernel clock beside them
  python tools/gemm_time.py --rt [3] [4]                f32x6 only: the tiles (values of MDD_GEMM_X6_RT; default 3 4) as the arms, in the same
        [--raster ARM] [--rows M ...]                   way (at least three visits), under one walk (default: the library's); --rows: the row
                                                        counts to time at K = 1952 and 768 (default 128000, 16000)
The in-kernel clock is the median over workgroups of (shader-clock ticks) / (ticks of the 100 MHz constant clock) x 100 MHz, stamped once
around the tile loop of the diagnostic instantiation; the production kernel carries no stamp."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from ctc_attention_mispronunciation_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("modes", nargs="*", type=int)
ap.add_argument("--raster", nargs="*", default=None, metavar="ARM")
ap.add_argument("--rt", nargs="*", default=None, metavar="RT")
ap.add_argument("--rows", nargs="*", type=int, default=None, metavar="M")
ap.add_argument("--cycles", type=int, default=5)
ap.add_argument("--seconds", type=float, default=2.0)
args = ap.parse_args()

L = _lib.lib()
torch.zeros(1).cuda()
L.mdd_diag_gemm_time.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
names = {0: "exact fp32 MFMA", 1: "split-bf16 x3", 3: "f32x6"}
peak = {0: 157.3, 1: 2500.0 / 3, 3: 2500.0 / 6}

if args.raster is None and args.rt is None:
    shapes = [(128000, 3072, 1952), (128000, 3072, 768), (20480, 3072, 512)]
    for M, N, K in shapes:
        for mode in args.modes or [0, 1, 3]:
            ms = C.c_float(0)
            rc = L.mdd_diag_gemm_time(mode, M, N, K, 5, C.byref(ms))
            assert rc == 0, L.mdd_last_error().decode()
            tf = 2.0 * M * N * K / (ms.value * 1e-3) / 1e12
            print("%7d x %4d x %4d  %-16s %8.3f ms  %7.1f TFLOP/s algorithmic  (%.2f of this arithmetic's matrix-core ceiling)" % (M, N, K, names[mode], ms.value, tf, tf / peak[mode]))
    sys.exit(0)

L.mdd_diag_gemm_clock.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
if args.rt is not None:     # the tiles as the arms, under one walk
    switch, arms, cycles = "MDD_GEMM_X6_RT", args.rt or ["3", "4"], max(3, args.cycles)
    assert not args.raster or len(args.raster) == 1, "--rt takes one walk"
    if args.raster:
        os.environ["MDD_GEMM_X6_RASTER"] = args.raster[0]
    first = "3"
else:
    switch, arms, cycles, first = "MDD_GEMM_X6_RASTER", args.raster or ["rows", "2x16", "4x8", "8x4"], args.cycles, "rows"
label = "RT=%s" if args.rt is not None else "%s"
for M, N, K in [(m, 3072, k) for m in (args.rows or ([128000, 16000] if args.rt is not None else [128000])) for k in (1952, 768)]:
    os.environ[switch] = first
    ms = C.c_float(0)
    assert L.mdd_diag_gemm_time(3, M, N, K, 5, C.byref(ms)) == 0, L.mdd_last_error().decode()
    reps = max(5, int(args.seconds * 1e3 / ms.value))
    seen = {a: [] for a in arms}
    for cyc in range(cycles):
        for a in arms:
            os.environ[switch] = a
            mhz = C.c_float(0)
            assert L.mdd_diag_gemm_clock(M, N, K, reps, C.byref(ms), C.byref(mhz)) == 0, L.mdd_last_error().decode()
            seen[a].append((ms.value, mhz.value))
            print("  visit %d  %-5s %8.4f ms  %6.0f MHz" % (cyc, label % a, ms.value, mhz.value), flush=True)
    for a in arms:
        t, f = [v[0] for v in seen[a]], [v[1] for v in seen[a]]
        med = statistics.median(t)
        tf = 2.0 * M * N * K / (med * 1e-3) / 1e12
        print("%7d x %4d x %4d  f32x6 %-5s  median %8.4f ms  min %8.4f ms  (%d visits x %d launches)  in-kernel clock median %6.0f MHz  %6.1f TFLOP/s algorithmic (%.2f of the ceiling)"
              % (M, N, K, label % a, med, min(t), len(t), reps, statistics.median(f), tf, tf / peak[3]), flush=True)
