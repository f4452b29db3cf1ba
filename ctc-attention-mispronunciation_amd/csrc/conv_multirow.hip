// The default fused conv front end of the f32x6 mode: CM_R output rows per pass, barrier-phased (its row-at-a-time yardstick: conv_fused.hip).
#include "conv_fused.h"

namespace mdd {

// ---------------------------------------------------------------- fused conv0 -> conv1, f32x6 form, R output rows per pass
// The same arithmetic as conv_fused_kernel<3> (the same six products in the same order per MFMA, the same MFMA shapes and k order, the
// two K halves accumulated apart and added last), reorganised so that the per-row bookkeeping around the small MFMA groups is paid
// once per R output rows:
//  * the x tile holds the 2R+3 x rows of R output rows (2tp-2 .. 2tp+2R); the next block's rows are requested right after conv0 has
//    read the tile, so they travel while conv1 runs instead of queueing behind the output stores;
//  * the conv0 tile holds 2R+1 rows in rotating slots; after a segment's first block only its 2R new rows are computed (R x 122
//    positions = 4 tiles of 32 per wave, one unrolled group);
//  * 8 waves, two per SIMD; conv1: wave = (output row jr, M tile mt, K half kh2) with its 9 k-steps of W1's three planes resident.  (All of
//    K per wave needs 216 registers for W1 alone: measured slower, the rest of the kernel then lives in AGPR copies --
//    profiles/round4_conv_notes.txt.)  The block is barrier-phased: all waves are in conv0 (vector work) or in conv1 (matrix work) together,
//    so what counts is the number of instructions around the MFMAs (profiles/conv_pipeline_notes.txt):
//  * nothing that depends only on the thread is computed in the row loop: which x elements a thread fetches (the stack/skip index map of
//    raw frames included; the fetch is a buffer load whose out-of-range elements read as zero), where its 16-byte output chunks go, the
//    column part of its conv1 fragment addresses; the wave index is a scalar, so the row slots, the K half and the output row are scalar;
//  * every three-plane split (x operand, conv0 output, conv1 output) converts two values per instruction (split3_pair);
//  * the conv1 epilogue is shared by the two K halves of a tile: each hands the other 8 of its 16 partial sums and finishes the other 8;
//  * the R output rows are transposed into LDS together and written as 16-byte granules of the K-tile-major planes.

// Three-plane split of two values at a time, the arithmetic of the scalar casts (round to nearest even, exact residuals): one packed
// conversion per plane; a bf16 back to fp32 is a shift (low half = a) or a mask (high half = b) of the packed word (as lstm_x6.hip)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
// The residuals are single v_sub_f32: left to itself the compiler pairs neighbouring ones into v_pk_add_f32, which measured slower around
// these MFMAs (profiles/conv_pipeline_notes.txt).
__device__ __forceinline__ float sub_f32(float a, float b) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ void split3_pair(float a, float b, unsigned &h, unsigned &m, unsigned &l) {
    h = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2));
    const float a1 = sub_f32(a, __builtin_bit_cast(float, h << 16)), b1 = sub_f32(b, __builtin_bit_cast(float, h & 0xffff0000u));
    m = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a1, b1}, bf16x2));
    const float a2 = sub_f32(a1, __builtin_bit_cast(float, m << 16)), b2 = sub_f32(b1, __builtin_bit_cast(float, m & 0xffff0000u));
    l = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a2, b2}, bf16x2));
}

__device__ __forceinline__ int cm_yoff(int slot, int col, int chunk) { return (slot * CF_NCOL + col) * 64 + ((chunk ^ ((col >> 2) & 3)) << 4); }

// STAMP (diagnostic instantiation, mdd_diag_conv_time): per wave, cycle sums of the CM_NPH phases of a block -> stamps[(workgroup * 8 +
// wave) * CM_NPH + phase] for the first 512 workgroups: 0 wait for the previous block's readers, 1 x tile store, 2 barrier, 3 conv0 and the
// next x request, 4 barrier, 5 conv1 and the K-half partials, 6 barrier, 7 conv1 epilogue, 8 barrier, 9 row stores (tools/conv_stamps.py)
template <int NP, int R, bool STAMP>
__global__ __launch_bounds__(512, 1) void conv_fused_kernel(const float *__restrict__ x, const float *__restrict__ w0,
                                                            const float *__restrict__ sc0, const float *__restrict__ sh0,
                                                            const unsigned short *__restrict__ w1_3, const float *__restrict__ sc1,
                                                            const float *__restrict__ sh1, unsigned short *__restrict__ out3,
                                                            float *__restrict__ out_f32, int B, int T, int Traw, int S, int seg,
                                                            long long *stamps) {
    static_assert(NP == 3 && R == CM_R, "multi-row form: f32x6 planes, CM_R rows (LDS layout above)");
    long long sacc[CM_NPH] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, stt = 0;
#define CM_T(i_) do { if (STAMP) { const long long n_ = (long long)__builtin_readcyclecounter(); sacc[i_] += n_ - stt; stt = n_; } } while (0)
    constexpr int F = 243, W1 = 122, W2 = 61, CH = 32, ROW = CH * W2;   // 1952
    constexpr int D0 = F / 3;
    constexpr int NY = 2 * R + 1, NX = 2 * R + 3;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *yh = smem, *ym = yh + CM_YPLANE, *yl = ym + CM_YPLANE;
    float *xs = reinterpret_cast<float *>(yl + CM_YPLANE);                         // [NX][CF_XLD]
    unsigned short *ost = reinterpret_cast<unsigned short *>(yl + CM_YPLANE);      // [R][hi, mid, lo][ROW] (after conv0 has read xs)
    float *red = reinterpret_cast<float *>(yl + CM_YPLANE + (CM_XT > CM_OST ? CM_XT : CM_OST));   // [2R tiles][16][64]
    float *bn0 = red + CM_RED / 4;                                                 // conv0's folded BN: scale [32] | shift [32]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                   // scalar: roles, row slots and row bases cost no vector work
    const int li = lane & 31, half = lane >> 5;
    const int kh2 = wave >> 2, jr = (wave >> 1) & 1, mt = wave & 1;              // conv1: output row tp + jr, M tile mt, K half kh2
    const int Tp = T / 2;
    const size_t mrows = (size_t)Tp * B;

    // resident B fragments: W1[co = li][k], this wave's 9 k-steps of 16, three planes
    bf16x8 bwh[9], bwm[9], bwl[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const size_t o = (size_t)li * 288 + (kh2 * 9 + i) * 16 + half * 8;
        bwh[i] = *reinterpret_cast<const bf16x8 *>(w1_3 + o);
        bwm[i] = *reinterpret_cast<const bf16x8 *>(w1_3 + CH * 288 + o);
        bwl[i] = *reinterpret_cast<const bf16x8 *>(w1_3 + 2 * CH * 288 + o);
    }
    bf16x8 w0h, w0m, w0l;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int tap = half * 8 + j;
        const float wv = tap < 9 ? w0[li * 9 + tap] : 0.f;
        w0h[j] = (__bf16)wv;
        const float r1 = wv - (float)w0h[j];
        w0m[j] = (__bf16)r1; w0l[j] = (__bf16)(r1 - (float)w0m[j]);
    }
    if (tid < 64) bn0[tid] = tid < 32 ? sc0[tid] : sh0[tid - 32];               // (read behind the loop's first barrier)
    const float s1 = sc1[li], h1 = sh1[li];
    // zero the left pad column (col 0 = conv0 column -1) of every slot of the three planes once
    for (int i = tid; i < 3 * NY * 16; i += 512) {
        const int pl = i / (NY * 16), rem = i - pl * (NY * 16);
        reinterpret_cast<unsigned int *>(smem + pl * CM_YPLANE + (rem >> 4) * CF_NCOL * 64)[rem & 15] = 0u;
    }

    const int b = blockIdx.x / S, sidx = blockIdx.x - b * S;                      // utterance b, segment sidx of S
    const int tp_begin = sidx * seg, tp_end = min(Tp, tp_begin + seg);
    constexpr int XPT = (NX * CF_XLD + 511) / 512;
    // x rows 2tp-2 .. 2tp+2R, columns -1 .. 246 (zero outside) of a block.  What a thread's XPT elements are does not depend on the block:
    // tile row xr (a row no utterance has for an element outside the tile or the feature columns), frame term xq and byte offset xo in the
    // frame are computed once.  Element (row ti = 2tp - 2 + xr) then lives in frame min(fa * (2tp - 2) + xq, flim) of the utterance --
    // stacked features: the row itself (fa = 1, xq = xr); raw frames (see conv_fused_kernel<NP>): fa = 2, xq = 2 xr + j for third j of the
    // stacked row, clamped to the last frame -- and rows outside [0, tlim) are zero.  The utterance is a buffer resource: an element that
    // is not to be read gets an offset past its end and reads as zero, without a branch.
    const int fa = Traw == 0 ? 1 : 2, flim = Traw == 0 ? T - 1 : Traw - 1, tlim = Traw == 0 ? T : (Traw + 1) / 2;
    const int fbytes = (Traw == 0 ? F : D0) * 4;
    int xr[XPT], xq[XPT], xo[XPT];
#pragma unroll
    for (int k = 0; k < XPT; k++) {
        const int i = tid + 512 * k, r = i / CF_XLD, c = i - r * CF_XLD - 1, j = Traw == 0 ? 0 : c / D0;
        xr[k] = (i < NX * CF_XLD && c >= 0 && c < F) ? r : 0x20000000;
        xq[k] = fa * r + j;
        xo[k] = (c - j * D0) * 4;
    }
    const auto xrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(x) + (size_t)b * (Traw == 0 ? T : Traw) * (Traw == 0 ? F : D0), 0, (flim + 1) * fbytes, 0x00020000);
    auto load_x = [&](int tp, float (&dst)[XPT]) {
        const int t0 = 2 * tp - 2, f0 = fa * t0;
#pragma unroll
        for (int k = 0; k < XPT; k++) {
            const int fr = min(f0 + xq[k], flim);
            const unsigned off = (unsigned)(t0 + xr[k]) < (unsigned)tlim ? (unsigned)(fr * fbytes + xo[k]) : 0xffffffffu;
            dst[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, off, 0, 0));
        }
    };
    // row stores: chunk i = tid + 512 k of a block's staged rows is (row jj, plane pl, 16-byte chunk q); where it goes, but for the
    // block's row base, is computed once
    constexpr int SPT = (R * 3 * 244 + 511) / 512;
    size_t sdst[SPT];
#pragma unroll
    for (int k = 0; k < SPT; k++) {
        const int i = tid + 512 * k, jj = i / (3 * 244), rem = i - jj * (3 * 244), pl = rem / 244, q = rem - pl * 244;
        sdst[k] = pl * mrows * ROW + ((size_t)(q >> 2) * mrows + (size_t)jj * B + b) * 32 + (q & 3) * 8;
    }
    float xnext[XPT];
    if (tp_begin < tp_end) load_x(tp_begin, xnext);
    int rot = 0;                                                                   // logical conv0 row r lives in slot (r + rot) % NY
    if (STAMP) stt = (long long)__builtin_readcyclecounter();
    for (int tp = tp_begin; tp < tp_end; tp += R) {
        const bool fresh = tp == tp_begin;
        if (!fresh) rot = rot == 0 ? NY - 1 : rot - 1;                             // old logical row NY-1 becomes row 0
        __syncthreads();                                                           // previous block's tile and staged rows consumed
        CM_T(0);
#pragma unroll
        for (int k = 0; k < XPT; k++) if (tid + 512 * k < NX * CF_XLD) xs[tid + 512 * k] = xnext[k];
        CM_T(1);
        __syncthreads();
        CM_T(2);
        // ---- conv0 (as in conv_fused_kernel<3>): logical rows 0 .. NY-1 = conv0 rows 2tp-1 .. 2tp+2R-1; positions p = r * W1 + wc
        auto conv0_tile = [&](int p) {
            const int pc = min(p, NY * W1 - 1);
            const int r = pc / W1, wc = pc - r * W1, ti = 2 * tp - 1 + r;
            const int rs = r + rot >= NY ? r + rot - NY : r + rot;
            const bool inb = p < NY * W1;
            // a conv0 row outside the utterance is zero: a property of the row, so it goes into the ReLU's threshold (nothing exceeds +inf)
            const float thr = (ti >= 0 && ti < T && inb) ? 0.f : __builtin_inff();
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int tap = half * 8 + j, kh = tap / 3, kw = tap - kh * 3;
                v[j] = (tap < 9) ? xs[(r + kh) * CF_XLD + 2 * wc + kw] : 0.f;
            }
            u32x4 ph, pm, pl;
#pragma unroll
            for (int j = 0; j < 4; j++) { unsigned h_, m_, l_; split3_pair(v[2 * j], v[2 * j + 1], h_, m_, l_); ph[j] = h_; pm[j] = m_; pl[j] = l_; }
            const bf16x8 bh = __builtin_bit_cast(bf16x8, ph), bm = __builtin_bit_cast(bf16x8, pm), bl = __builtin_bit_cast(bf16x8, pl);
            f32x16 d;
#pragma unroll
            for (int q = 0; q < 16; q++) d[q] = 0.f;
            d = conv_products<3>(w0h, w0m, w0l, bh, bm, bl, d);
            if (inb) {
#pragma unroll
                for (int g = 0; g < 4; g++) {      // registers 4g..4g+3 = channels 8g + 4*half + 0..3 = 16-byte chunk g, bytes 8*half..
                    const float4 c0s = *reinterpret_cast<const float4 *>(bn0 + 8 * g + 4 * half);
                    const float4 c0h = *reinterpret_cast<const float4 *>(bn0 + 32 + 8 * g + 4 * half);
                    const float cs[4] = {c0s.x, c0s.y, c0s.z, c0s.w}, chh[4] = {c0h.x, c0h.y, c0h.z, c0h.w};
                    float a[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        a[e] = d[4 * g + e] * cs[e] + chh[e];
                        a[e] = a[e] > thr ? a[e] : 0.f;
                    }
                    uint2 hw, mw, lw;
                    split3_pair(a[0], a[1], hw.x, mw.x, lw.x);
                    split3_pair(a[2], a[3], hw.y, mw.y, lw.y);
                    const int o = cm_yoff(rs, wc + 1, g) + 8 * half;
                    *reinterpret_cast<uint2 *>(yh + o) = hw;
                    *reinterpret_cast<uint2 *>(ym + o) = mw;
                    *reinterpret_cast<uint2 *>(yl + o) = lw;
                }
            }
        };
        {   // a fresh block computes all NY rows (5 x 122 positions = 20 tiles), a continuing one the 2R new rows (16 tiles; row 0 is
            // the previous block's row NY-1)
            const int p0 = fresh ? 0 : W1;
            conv0_tile(p0 + wave * 32 + li);
            conv0_tile(p0 + (wave + 8) * 32 + li);
            if (fresh && wave < 4) conv0_tile((16 + wave) * 32 + li);
        }
        if (tp + R < tp_end) load_x(tp + R, xnext);                                // the next block's x rows travel during conv1
        CM_T(3);
        __syncthreads();
        CM_T(4);
        // ---- conv1: this wave = output row tp + jr (logical conv0 rows 2jr .. 2jr+2), M tile mt, k-steps 9 kh2 .. 9 kh2 + 8
        // (the K half is a template argument of the two lambdas below: tap, chunk and accumulator register of every step are constants)
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
        const int m = min(mt * 32 + li, W2 - 1);                                   // rows >= 61 recompute row 60, never stored
        int slot[3];                                                               // scalar: byte offset of the slot of conv0 row 2jr + kh
#pragma unroll
        for (int kh = 0; kh < 3; kh++) { const int r = 2 * jr + kh + rot; slot[kh] = (r >= NY ? r - NY : r) * CF_NCOL * 64; }
        float *rt = red + (jr * 2 + mt) * 16 * 64;
        // Each K half finishes 8 of the tile's 16 accumulator registers (half 0: registers 0..7 = w' 0..3, 8..11 (+4 by lane half) of the
        // tile; half 1: 8..15) and hands the other 8 to its partner through rt: no wave waits out the epilogue at the barrier.
        auto conv1 = [&](auto kc) {
            constexpr int KH2 = decltype(kc)::value;
#pragma unroll
            for (int i = 0; i < 9; i++) {
                const int kb = KH2 * 9 + i, kk = kb >> 1, kh = kk / 3, kw = kk - kh * 3;
                const int off = slot[kh] + cm_yoff(0, 2 * m + kw, (kb & 1) * 2 + half);   // col index = (2m+kw-1)+1
                const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(yh + off);
                const bf16x8 am = *reinterpret_cast<const bf16x8 *>(ym + off);
                const bf16x8 al = *reinterpret_cast<const bf16x8 *>(yl + off);
                acc = conv_products<3>(ah, am, al, bwh[i], bwm[i], bwl[i], acc);
            }
#pragma unroll
            for (int r = 0; r < 8; r++) rt[((1 - KH2) * 8 + r) * 64 + lane] = acc[(1 - KH2) * 8 + r];
        };
        // ---- sum of the K halves (half 0 + half 1, as the row-wise kernel adds them), BN + ReLU + three-plane split, transposed into the
        // staged output row jr (xs is dead: the barrier above followed conv0)
        auto finish = [&](auto kc) {
            constexpr int KH2 = decltype(kc)::value;
            unsigned short *oh = ost + jr * 3 * ROW + li * W2 + mt * 32 + 4 * half, *om = oh + ROW, *ol = om + ROW;
            const bool cut = mt == 1 && half == 1;                                 // w' = 60 + (r & 3) of registers 12..15: only w' = 60 exists
#pragma unroll
            for (int r = KH2 * 8; r < KH2 * 8 + 8; r += 2) {                       // C/D: row = w' = mt*32 + (r&3) + 8*(r>>2) + 4*half, col = li = co
                float v[2];
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const float p = rt[(r + e) * 64 + lane];
                    v[e] = (KH2 == 0 ? acc[r + e] + p : p + acc[r + e]) * s1 + h1;
                    v[e] = v[e] > 0.f ? v[e] : 0.f;
                }
                unsigned hw, mw, lw;
                split3_pair(v[0], v[1], hw, mw, lw);
                const int wo = (r & 3) + 8 * (r >> 2);
                if (r < 13 || !cut) { oh[wo] = (unsigned short)hw; om[wo] = (unsigned short)mw; ol[wo] = (unsigned short)lw; }
                if (r + 1 < 13 || !cut) { oh[wo + 1] = (unsigned short)(hw >> 16); om[wo + 1] = (unsigned short)(mw >> 16); ol[wo + 1] = (unsigned short)(lw >> 16); }
            }
        };
        if (kh2 == 0) conv1(std::integral_constant<int, 0>{}); else conv1(std::integral_constant<int, 1>{});
        CM_T(5);
        __syncthreads();
        CM_T(6);
        if (tp + jr < tp_end) {
            if (kh2 == 0) finish(std::integral_constant<int, 0>{}); else finish(std::integral_constant<int, 1>{});
        }
        CM_T(7);
        __syncthreads();
        CM_T(8);
        // ---- stores: 16-byte chunk q of plane pl of staged row jj = columns 8q .. 8q+7 = K-tile q / 4, offset (q % 4) * 8; chunk i of the
        // staged rows sits at element 8 i, and its destination is the thread's own constant plus the block's row base
        const int nr = min(R, tp_end - tp);
        unsigned short *orow = out3 + (size_t)tp * B * 32;
#pragma unroll
        for (int k = 0; k < SPT; k++) {
            const int i = tid + 512 * k;
            if (i < nr * 3 * 244) *reinterpret_cast<u32x4 *>(orow + sdst[k]) = *reinterpret_cast<const u32x4 *>(ost + i * 8);
        }
        if (out_f32)
            for (int i = tid; i < nr * ROW; i += 512) {
                const int jj = i / ROW, c = i - jj * ROW;
                const unsigned short *oh = ost + jj * 3 * ROW;
                out_f32[((size_t)(tp + jj) * B + b) * ROW + c] =
                    (__uint_as_float((unsigned)oh[c] << 16) + __uint_as_float((unsigned)oh[ROW + c] << 16)) + __uint_as_float((unsigned)oh[2 * ROW + c] << 16);
            }
        CM_T(9);
    }
    if (STAMP && stamps && lane == 0 && blockIdx.x < 512)
        for (int i = 0; i < CM_NPH; i++) stamps[((size_t)blockIdx.x * 8 + wave) * CM_NPH + i] = sacc[i];
#undef CM_T
}

// f32x6 form: w1_3 = conv1 weights [co][kh][kw][ci] as three consecutive row-major planes (hi | mid | lo, 32 * 288 elements each);
// out3 = three consecutive K-tile-major planes of (T/2 * B) x 1952 elements (the A operand of launch_gemm_f32x6)
// rowwise: the row-at-a-time kernel (MDD_CONV=rowwise, diagnostic); otherwise conv_fused_kernel<3, CM_R>, bit-identical to it.
int launch_conv_fused3(const float *x, const float *w0, const float *sc0, const float *sh0, const unsigned short *w1_3, const float *sc1,
                       const float *sh1, unsigned short *out3, float *out_f32, int B, int T, int Traw, hipStream_t st, bool rowwise,
                       long long *stamps) {
    const int Tp = T / 2;
    if (Tp <= 0 || B <= 0) return MDD_OK;
    if (rowwise) return launch_conv_fused3_rowwise(x, w0, sc0, sh0, w1_3, sc1, sh1, out3, out_f32, B, T, Traw, st);
    const auto [S, seg] = conv_segments(B, Tp, 512, CM_R);
    if (stamps) hipLaunchKernelGGL((conv_fused_kernel<3, CM_R, true>), dim3(B * S), dim3(512), conv_multirow_smem(), st, x, w0, sc0, sh0, w1_3,
                                   sc1, sh1, out3, out_f32, B, T, Traw, S, seg, stamps);
    else hipLaunchKernelGGL((conv_fused_kernel<3, CM_R, false>), dim3(B * S), dim3(512), conv_multirow_smem(), st, x, w0, sc0, sh0, w1_3,
                            sc1, sh1, out3, out_f32, B, T, Traw, S, seg, nullptr);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

int init_conv_multirow_attributes() {
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)conv_fused_kernel<3, CM_R, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)conv_multirow_smem()));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)conv_fused_kernel<3, CM_R, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)conv_multirow_smem()));
    return MDD_OK;
}

}  // namespace mdd
