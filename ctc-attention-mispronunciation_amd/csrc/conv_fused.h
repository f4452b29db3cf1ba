// What the two fused conv0 -> conv1 kernels share (conv_fused.hip: row at a time; conv_multirow.hip: CM_R rows per pass): vector types, LDS
// layout constants, the segment geometry of their launches and the device pieces both write the same way.
#pragma once
#include "mdd_internal.h"

namespace mdd {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// (row-wise kernel)
// LDS: x tile [5][248] f32 | y0 hi/lo [3][124 cols][80 B] (32 ch x bf16 + 16 B pad: 2-way-conflict fragment reads)
//      | K-half reduction [2][32x32] f32 | output row [1952] hi, lo.
constexpr int CF_XLD = 248, CF_COLB = 80, CF_NCOL = 124, CF_YPLANE = 3 * CF_NCOL * CF_COLB;   // 29760 B
size_t conv_fused_smem(int np);

// (multi-row kernel)
// LDS (R = 2): conv0 tile 3 planes x [5 slots][124 cols][64 B] (32 channels bf16; the four 16-byte chunks of a column are XOR-swizzled
// by column bits 2..3: 2-way-conflict fragment reads, as the padded layout of the row-wise kernel) | x tile [7][248] f32, whose bytes
// later stage the output rows [R][3 planes][1952] | K-half partial sums [2R tiles][16][64] f32 | conv0's folded BN (kept out of
// registers: with it there the kernel spills).
constexpr int CM_R = 2, CM_NY = 2 * CM_R + 1, CM_NX = 2 * CM_R + 3;
constexpr int CM_YPLANE = CM_NY * CF_NCOL * 64;                                    // 39680 B
constexpr int CM_XT = CM_NX * CF_XLD * 4, CM_OST = CM_R * 3 * 1952 * 2;             // 6944 B, 23424 B
constexpr int CM_RED = 2 * CM_R * 16 * 64 * 4;                                      // 16384 B: K-half partial sums of the 2R output tiles
constexpr size_t conv_multirow_smem() { return 3 * (size_t)CM_YPLANE + (CM_XT > CM_OST ? CM_XT : CM_OST) + CM_RED + 256; }   // 159104 B

// Segments of consecutive output rows per utterance: about `target` workgroups over the B utterances (1024: two rounds of the 512 that fit
// the chip; 512: one workgroup per CU at 114 / 159 KB of LDS, two rounds of 256), seg rows each, in whole blocks of `block` rows except at
// the utterance's end, no empty segments.  Tp, B > 0.
struct ConvSegments { int S, seg; };
inline ConvSegments conv_segments(int B, int Tp, int target, int block) {
    int S = (target + B - 1) / B;
    S = S < 1 ? 1 : (S > Tp ? Tp : S);
    const int seg = ((Tp + S - 1) / S + block - 1) / block * block;
    return {(Tp + seg - 1) / seg, seg};
}

// The product group of one MFMA k-step, smallest products first, into acc: A = ah + am + al, B = bh + bm + bl; NP = 3 the five small products
// then hi.hi, NP = 2 (no mid plane: am, bm unused) hi.lo, lo.hi then hi.hi.  conv0 (A = weights) and conv1 (B = weights) of both kernels.
template <int NP>
__device__ __forceinline__ f32x16 conv_products(bf16x8 ah, bf16x8 am, bf16x8 al, bf16x8 bh, bf16x8 bm, bf16x8 bl, f32x16 acc) {
    if (NP == 3) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

// conv_fused.hip <-> conv_multirow.hip (hidden: the exported symbols stay as they were)
__attribute__((visibility("hidden"))) int launch_conv_fused3_rowwise(const float *x, const float *w0, const float *sc0, const float *sh0,
                                                                     const unsigned short *w1_3, const float *sc1, const float *sh1, unsigned short *out3,
                                                                     float *out_f32, int B, int T, int Traw, hipStream_t st);
__attribute__((visibility("hidden"))) int init_conv_multirow_attributes();

}  // namespace mdd
