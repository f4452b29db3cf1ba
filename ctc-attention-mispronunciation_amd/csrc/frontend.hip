// Input stacking and the 2-layer CNN front-end.
//
// Reference: make_context/skip_feat (AA/utils/tools.py:207-227, AA/utils/data_loader.py:138-142) and
// LayerCNN.forward x2 (AA/models/model_ctc.py:73-81; geometry AA/conf/ctc_config.0329.yaml:59-64):
//   conv0: Conv2d(1->ch, k3x3, stride (1,2), pad 1) + bias -> BN2d(eval) -> ReLU
//   conv1: Conv2d(ch->ch, k3x3, stride (2,2), pad 1) + bias -> BN2d(eval) -> ReLU
// followed by the [B,ch,T',W2] -> [T',B,ch*W2] relayout (model_ctc.py:176-181), which conv1's store
// performs directly.  Eval BatchNorm and the conv bias are folded into per-channel scale/shift on
// the host side of the library (y = conv_nobias * scale + shift).
#include "mdd_internal.h"

namespace mdd {

// ---------------------------------------------------------------- A1
__global__ void stack_skip_kernel(const float *__restrict__ raw, int T_raw, int D, int right, int skip, int kept,
                                  int T_out, float *__restrict__ out) {
    const int W = (right + 1) * D;
    const int b = blockIdx.y, i = blockIdx.x;  // one output frame per block
    const float *src = raw + (size_t)b * T_raw * D;
    float *dst = out + ((size_t)b * T_out + i) * W;
    for (int j = threadIdx.x; j < W; j += blockDim.x) {
        float v = 0.f;
        if (i < kept) {
            int r = j / D, c = j - r * D;
            int s = i * skip + r;
            if (s > T_raw - 1) s = T_raw - 1;  // last frame replicated at the edge
            v = src[(size_t)s * D + c];
        }
        dst[j] = v;
    }
}

int launch_stack_skip(const float *raw, int B, int T_raw, int D, int right, int skip, int n_down, float *out,
                      hipStream_t st) {
    if (B <= 0 || T_raw <= 0 || D <= 0 || right < 0) { set_error("stack_skip: bad shape"); return MDD_ERR_ARG; }
    if (skip < 1) skip = 1;
    int kept = (T_raw + skip - 1) / skip;
    int T_out = mdd_stack_len(T_raw, skip, n_down);
    hipLaunchKernelGGL(stack_skip_kernel, dim3(T_out, B), dim3(256), 0, st, raw, T_raw, D, right, skip, kept, T_out, out);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// ---------------------------------------------------------------- conv0 (Cin = 1)
// one thread per output position (b,t,w), all channels; stores are coalesced over w per channel.
template <int CH>
__global__ __launch_bounds__(256) void conv0_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                    const float *__restrict__ scale, const float *__restrict__ shift,
                                                    float *__restrict__ y, int B, int T, int F, int W1) {
    const int wo = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = blockIdx.y, b = blockIdx.z;
    if (wo >= W1) return;
    float in[3][3];
#pragma unroll
    for (int kh = 0; kh < 3; kh++) {
        int ti = t + kh - 1;
#pragma unroll
        for (int kw = 0; kw < 3; kw++) {
            int fi = wo * 2 + kw - 1;
            in[kh][kw] = (ti >= 0 && ti < T && fi >= 0 && fi < F) ? x[((size_t)b * T + ti) * F + fi] : 0.f;
        }
    }
#pragma unroll 4
    for (int c = 0; c < CH; c++) {
        float acc = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; kh++)
#pragma unroll
            for (int kw = 0; kw < 3; kw++) acc = fmaf(in[kh][kw], w[c * 9 + kh * 3 + kw], acc);
        float v = acc * scale[c] + shift[c];
        y[(((size_t)b * CH + c) * T + t) * W1 + wo] = v > 0.f ? v : 0.f;
    }
}

int launch_conv0(const float *x, const float *w, const float *scale, const float *shift, float *y0, int B, int T, int F,
                 int ch, hipStream_t st) {
    int W1 = (F + 2 - 3) / 2 + 1;
    dim3 grid((W1 + 127) / 128, T, B), block(128);
    if (ch == 32) hipLaunchKernelGGL(conv0_kernel<32>, grid, block, 0, st, x, w, scale, shift, y0, B, T, F, W1);
    else if (ch == 4) hipLaunchKernelGGL(conv0_kernel<4>, grid, block, 0, st, x, w, scale, shift, y0, B, T, F, W1);
    else { set_error("conv0: channels=%d not built (32 or 4)", ch); return MDD_ERR_ARG; }
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// ---------------------------------------------------------------- conv1 (CH -> CH, stride 2x2)
// Weights are pre-transposed on load to w_t[ci][kh][kw][co] and staged in LDS; every lane reads the
// same 16-byte slot (broadcast).  A thread produces all CH output channels for two adjacent output
// columns so each broadcast weight read feeds two FMAs.
template <int CH>
__global__ __launch_bounds__(256) void conv1_kernel(const float *__restrict__ y0, const float *__restrict__ w_t,
                                                    const float *__restrict__ scale, const float *__restrict__ shift,
                                                    float *__restrict__ seq, unsigned short *__restrict__ seq_hi,
                                                    unsigned short *__restrict__ seq_lo, int B, int T, int W1, int W2) {
    __shared__ __attribute__((aligned(16))) float wl[CH * 9 * CH];
    for (int i = threadIdx.x; i < CH * 9 * CH; i += blockDim.x) wl[i] = w_t[i];
    __syncthreads();
    const int Tp = T / 2, pairs = (W2 + 1) / 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // (output row, pair of output columns)
    const int tp = idx / pairs, b = blockIdx.z;
    const int wo = (idx - tp * pairs) * 2;
    if (tp >= Tp) return;
    float acc0[CH], acc1[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) { acc0[c] = 0.f; acc1[c] = 0.f; }
    for (int ci = 0; ci < CH; ci++) {
        const float *plane = y0 + ((size_t)b * CH + ci) * T * W1;
#pragma unroll
        for (int kh = 0; kh < 3; kh++) {
            const int ti = tp * 2 + kh - 1;
            float in[5];
#pragma unroll
            for (int j = 0; j < 5; j++) {
                int fi = wo * 2 + j - 1;
                in[j] = (ti >= 0 && ti < T && fi >= 0 && fi < W1) ? plane[(size_t)ti * W1 + fi] : 0.f;
            }
#pragma unroll
            for (int kw = 0; kw < 3; kw++) {
                const float *wr = wl + ((ci * 3 + kh) * 3 + kw) * CH;
#pragma unroll
                for (int c = 0; c < CH; c += 4) {
                    float4 w4 = *reinterpret_cast<const float4 *>(wr + c);
                    acc0[c] = fmaf(in[kw], w4.x, acc0[c]);         acc1[c] = fmaf(in[kw + 2], w4.x, acc1[c]);
                    acc0[c + 1] = fmaf(in[kw], w4.y, acc0[c + 1]); acc1[c + 1] = fmaf(in[kw + 2], w4.y, acc1[c + 1]);
                    acc0[c + 2] = fmaf(in[kw], w4.z, acc0[c + 2]); acc1[c + 2] = fmaf(in[kw + 2], w4.z, acc1[c + 2]);
                    acc0[c + 3] = fmaf(in[kw], w4.w, acc0[c + 3]); acc1[c + 3] = fmaf(in[kw + 2], w4.w, acc1[c + 3]);
                }
            }
        }
    }
    const size_t ob = ((size_t)tp * B + b) * CH * W2;
#pragma unroll
    for (int c = 0; c < CH; c++) {
        float v0 = acc0[c] * scale[c] + shift[c];
        float v1 = acc1[c] * scale[c] + shift[c];
        v0 = v0 > 0.f ? v0 : 0.f; v1 = v1 > 0.f ? v1 : 0.f;
        const size_t o = ob + c * W2 + wo;
        if (seq) { seq[o] = v0; if (wo + 1 < W2) seq[o + 1] = v1; }
        if (seq_hi) {   // split-bf16 planes for the bf16x3 input projection
            __bf16 h0 = (__bf16)v0, h1 = (__bf16)v1;
            __bf16 l0 = (__bf16)(v0 - (float)h0), l1 = (__bf16)(v1 - (float)h1);
            seq_hi[o] = *reinterpret_cast<unsigned short *>(&h0); seq_lo[o] = *reinterpret_cast<unsigned short *>(&l0);
            if (wo + 1 < W2) { seq_hi[o + 1] = *reinterpret_cast<unsigned short *>(&h1); seq_lo[o + 1] = *reinterpret_cast<unsigned short *>(&l1); }
        }
    }
}

int launch_conv1(const float *y0, const float *w_t, const float *scale, const float *shift, float *seq, SplitPtr sp, int B,
                 int T, int W1, int ch, hipStream_t st) {
    int W2 = (W1 + 2 - 3) / 2 + 1;
    int pairs = (W2 + 1) / 2;
    dim3 grid(((T / 2) * pairs + 255) / 256, 1, B), block(256);
    if (ch == 32) hipLaunchKernelGGL(conv1_kernel<32>, grid, block, 0, st, y0, w_t, scale, shift, seq, sp.hi, sp.lo, B, T, W1, W2);
    else if (ch == 4) hipLaunchKernelGGL(conv1_kernel<4>, grid, block, 0, st, y0, w_t, scale, shift, seq, sp.hi, sp.lo, B, T, W1, W2);
    else { set_error("conv1: channels=%d not built (32 or 4)", ch); return MDD_ERR_ARG; }
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// ---------------------------------------------------------------- fused conv0 -> conv1 (split-bf16 MFMA)
// One pass over x produces the BiLSTM input rows directly: conv0 (+BN+ReLU) is recomputed per output row into LDS
// (3 conv0 rows x 122 columns x 32 channels, bf16 hi/lo) and conv1 runs as an implicit GEMM on the bf16 matrix cores
//   out[w', co] = sum_k A[w', k] . W1[co, k],   k = (kh, kw, ci), K = 288,  M = 61 (two 32-row tiles),  N = 32
// with the bf16x3 product form.  The 500 MB-per-batch conv0 activation (y0) never exists in HBM: the kernel reads
// x once (5 rows per output row) and writes the [T'*B, 1952] split-bf16 rows the input projection consumes.
// A workgroup is persistent over output rows (grid-stride), so its W1 fragments stay in registers.
// LDS: x tile [5][248] f32 | y0 hi/lo [3][124 cols][80 B] (32 ch x bf16 + 16 B pad: 2-way-conflict fragment reads)
//      | K-half reduction [2][32x32] f32 | output row [1952] hi, lo.
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int CF_XLD = 248, CF_COLB = 80, CF_NCOL = 124, CF_YPLANE = 3 * CF_NCOL * CF_COLB;   // 29760 B

// NP = 2: the split-bf16 x3 form (operands as hi + lo, products hi.lo + lo.hi + hi.hi; output: two row-major planes).
// NP = 3: the fp32-grade form of the f32x6 mode (gemm_bf16x6.hip): every operand as hi + mid + lo = all 24 significand bits, the six
// products down to 2^-24 of a product, smallest first; the contractions here are short (9 taps; 288 / 2 per wave), so one accumulator
// does.  Output: three planes in the K-TILE-MAJOR order the f32x6 projection GEMM streams (plane[kt][row][32], kt = column / 32), i.e.
// the conv output never exists as fp32 and needs no split pass.  w1l holds the mid plane followed by the lo plane in that case.
template <int NP>
__global__ __launch_bounds__(256, NP == 2 ? 2 : 1) void conv_fused_kernel(const float *__restrict__ x, const float *__restrict__ w0,
                                                            const float *__restrict__ sc0, const float *__restrict__ sh0,
                                                            const unsigned short *__restrict__ w1h, const unsigned short *__restrict__ w1l,
                                                            const float *__restrict__ sc1, const float *__restrict__ sh1,
                                                            unsigned short *__restrict__ out_hi, unsigned short *__restrict__ out_lo,
                                                            float *__restrict__ out_f32, int B, int T, int Traw, int S, int seg) {
    constexpr int F = 243, W1 = 122, W2 = 61, CH = 32, ROW = CH * W2;   // 1952
    constexpr int D0 = F / 3;                                           // raw feature width when x holds unstacked frames
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *xs = reinterpret_cast<float *>(smem);                                   // [5][CF_XLD]
    unsigned char *yh = smem + 5 * CF_XLD * 4, *yl = yh + CF_YPLANE;               // conv0 tile, hi / lo
    unsigned char *ym = yl + CF_YPLANE;                                            // (NP = 3) mid
    float *red = reinterpret_cast<float *>(yl + (NP - 1) * CF_YPLANE);             // [2][1024]
    unsigned short *oh = reinterpret_cast<unsigned short *>(red + 2048), *ol = oh + ROW, *om = ol + ROW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mt = wave & 1, kh2 = wave >> 1;                                      // M tile, K half of this wave
    const int li = lane & 31, half = lane >> 5;
    const int Tp = T / 2;

    // resident B fragments: W1[co = li][k], this wave's 9 k-steps of 16
    bf16x8 bwh[9], bwl[9], bwm[NP == 3 ? 9 : 1];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int kb = kh2 * 9 + i;
        bwh[i] = *reinterpret_cast<const bf16x8 *>(w1h + (size_t)li * 288 + kb * 16 + half * 8);
        if (NP == 3) {
            bwm[i] = *reinterpret_cast<const bf16x8 *>(w1l + (size_t)li * 288 + kb * 16 + half * 8);
            bwl[i] = *reinterpret_cast<const bf16x8 *>(w1l + (size_t)CH * 288 + (size_t)li * 288 + kb * 16 + half * 8);
        } else bwl[i] = *reinterpret_cast<const bf16x8 *>(w1l + (size_t)li * 288 + kb * 16 + half * 8);
    }
    // conv0 weights as resident A fragments: lane (channel li, k-slice half): taps half*8 .. half*8+7 (taps >= 9 are zero)
    bf16x8 w0h, w0l, w0m;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int tap = half * 8 + j;
        const float wv = tap < 9 ? w0[li * 9 + tap] : 0.f;
        w0h[j] = (__bf16)wv;
        const float r1 = wv - (float)w0h[j];
        if (NP == 3) { w0m[j] = (__bf16)r1; w0l[j] = (__bf16)(r1 - (float)w0m[j]); }
        else { w0l[j] = (__bf16)r1; w0m[j] = (__bf16)0.f; }
    }
    float c0s[16], c0h[16];      // folded BN of the 16 channels this lane receives in D: reg q -> channel (q&3) + 8*(q>>2) + 4*half
#pragma unroll
    for (int q = 0; q < 16; q++) { const int ch = (q & 3) + 8 * (q >> 2) + 4 * half; c0s[q] = sc0[ch]; c0h[q] = sh0[ch]; }
    // zero the left pad column of the conv0 tile once (wcol = -1)
    for (int i = tid; i < 3 * NP * CF_COLB / 4; i += 256) {
        const int r = i / (NP * CF_COLB / 4), rem = i - r * (NP * CF_COLB / 4), pl = rem / (CF_COLB / 4);
        reinterpret_cast<unsigned int *>((pl == 0 ? yh : pl == 1 ? yl : ym) + r * CF_NCOL * CF_COLB)[rem % (CF_COLB / 4)] = 0u;
    }

    // x rows 2tp-2 .. 2tp+2, columns -1 .. 243 (zero outside) of one output row: 5*248 elements, 5 per thread.  The next
    // row's elements are requested before this row's arithmetic starts and parked in registers (a row is otherwise a
    // chain global load -> LDS -> conv0 -> conv1 with the ~1 us load latency exposed every time).
    constexpr int XPT = (5 * CF_XLD + 255) / 256;
    auto load_x = [&](int tp, int b, float (&dst)[XPT]) {
#pragma unroll
        for (int k = 0; k < XPT; k++) {
            const int i = tid + 256 * k, r = i / CF_XLD, c = i - r * CF_XLD - 1, ti = 2 * tp - 2 + r;
            float v = 0.f;
            if (i < 5 * CF_XLD) {
                if (Traw == 0) {
                    if (ti >= 0 && ti < T && c >= 0 && c < F) v = x[((size_t)b * T + ti) * F + c];
                } else {   // x = raw frames [B, Traw, 81]: stacked frame ti = raw frames 2ti, 2ti+1, 2ti+2 (last frame repeated past the
                           // end, tools.py:207-220), frames 0, 2, 4, .. kept (:222-227), zero rows up to an even count (data_loader.py:140-142)
                    const int j = c / D0, fr = min(2 * ti + j, Traw - 1);
                    if (ti >= 0 && 2 * ti < Traw && c >= 0 && c < F) v = x[((size_t)b * Traw + fr) * D0 + (c - j * D0)];
                }
            }
            dst[k] = v;
        }
    };
    // A workgroup walks consecutive output rows tp of ONE utterance (segment sidx of S per utterance): conv0 row 2tp+1 of
    // one output row is conv0 row 2(tp+1)-1 of the next, so after the first row of a segment only two of the three conv0
    // rows are computed; the tile's three row slots rotate (logical row r lives in slot (r + rot) % 3).
    float xnext[XPT];
    const int b = blockIdx.x / S, sidx = blockIdx.x - b * S;
    const int tp_begin = sidx * seg, tp_end = min(Tp, tp_begin + seg);
    if (tp_begin < tp_end) load_x(tp_begin, b, xnext);
    int rot = 0;
    for (int tp = tp_begin; tp < tp_end; tp++) {
        const int rowid = tp * B + b;
        const bool fresh = tp == tp_begin;
        if (!fresh) rot = rot == 0 ? 2 : rot - 1;                                  // (rot + 2) % 3: old logical row 2 becomes row 0
        __syncthreads();                                                           // previous row's LDS fully consumed
#pragma unroll
        for (int k = 0; k < XPT; k++) if (tid + 256 * k < 5 * CF_XLD) xs[tid + 256 * k] = xnext[k];
        if (tp + 1 < tp_end) load_x(tp + 1, b, xnext);   // (all five x rows: skipping the one that only feeds the reused conv0 row costs more in branches than it saves)
        __syncthreads();
        // ---- conv0 on the matrix cores: D[ch, pos] = W0[ch, k] . P[k, pos], k = 9 taps padded to 16 (one MFMA k-step),
        // bf16x3.  A = weights (resident fragments), B = the 3x3 patch of each of the 3*122 = 366 positions (12 tiles of
        // 32, 3 per wave), built from the fp32 x tile.  D puts the position on the lane and 16 channels in the registers
        // (4 groups of 4 consecutive channels), exactly the [r][wcol+1][ci] rows conv1 reads: 8-byte LDS stores.
        for (int pt = wave; pt < (fresh ? 12 : 8); pt += 4) {
            const int p = (fresh ? 0 : W1) + pt * 32 + li, pc = min(p, 3 * W1 - 1);
            const int r = pc / W1, wc = pc - r * W1, ti = 2 * tp - 1 + r;
            const int rs = r + rot >= 3 ? r + rot - 3 : r + rot;                   // row slot in the tile
            const bool rowok = ti >= 0 && ti < T && p < 3 * W1;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int tap = half * 8 + j, kh = tap / 3, kw = tap - kh * 3;           // taps 9..15 are padding
                v[j] = (tap < 9) ? xs[(r + kh) * CF_XLD + 2 * wc + kw] : 0.f;
            }
            bf16x8 bh, bl, bm;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                bh[j] = (__bf16)v[j];
                const float r1 = v[j] - (float)bh[j];
                if (NP == 3) { bm[j] = (__bf16)r1; bl[j] = (__bf16)(r1 - (float)bm[j]); }
                else bl[j] = (__bf16)r1;
            }
            f32x16 d;
#pragma unroll
            for (int q = 0; q < 16; q++) d[q] = 0.f;
            if (NP == 3) {
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0m, bm, d, 0, 0, 0);
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0h, bl, d, 0, 0, 0);
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0l, bh, d, 0, 0, 0);
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0h, bm, d, 0, 0, 0);
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0m, bh, d, 0, 0, 0);
            } else {
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0h, bl, d, 0, 0, 0);
                d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0l, bh, d, 0, 0, 0);
            }
            d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0h, bh, d, 0, 0, 0);
            if (p < 3 * W1) {
                unsigned char *dh = yh + (rs * CF_NCOL + wc + 1) * CF_COLB, *dl = yl + (rs * CF_NCOL + wc + 1) * CF_COLB;
                unsigned char *dm = ym + (rs * CF_NCOL + wc + 1) * CF_COLB;
#pragma unroll
                for (int g = 0; g < 4; g++) {      // registers 4g..4g+3 = channels 8g + 4*half + 0..3
                    unsigned short hb[4], lb[4], mb[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        float a = d[4 * g + e] * c0s[4 * g + e] + c0h[4 * g + e];
                        a = (rowok && a > 0.f) ? a : 0.f;
                        __bf16 h = (__bf16)a;
                        const float r1 = a - (float)h;
                        hb[e] = *reinterpret_cast<unsigned short *>(&h);
                        if (NP == 3) {
                            __bf16 mm_ = (__bf16)r1, l = (__bf16)(r1 - (float)mm_);
                            mb[e] = *reinterpret_cast<unsigned short *>(&mm_); lb[e] = *reinterpret_cast<unsigned short *>(&l);
                        } else { __bf16 l = (__bf16)r1; lb[e] = *reinterpret_cast<unsigned short *>(&l); }
                    }
                    const int cb = (8 * g + 4 * half) * 2;
                    *reinterpret_cast<uint2 *>(dh + cb) = make_uint2(hb[0] | ((unsigned)hb[1] << 16), hb[2] | ((unsigned)hb[3] << 16));
                    *reinterpret_cast<uint2 *>(dl + cb) = make_uint2(lb[0] | ((unsigned)lb[1] << 16), lb[2] | ((unsigned)lb[3] << 16));
                    if (NP == 3) *reinterpret_cast<uint2 *>(dm + cb) = make_uint2(mb[0] | ((unsigned)mb[1] << 16), mb[2] | ((unsigned)mb[3] << 16));
                }
            }
        }
        __syncthreads();
        // ---- conv1: this wave = M tile mt (w' = mt*32 + li), K half kh2
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
        const int m = min(mt * 32 + li, W2 - 1);                                   // rows >= 61 recompute row 60, never stored
#pragma unroll
        for (int i = 0; i < 9; i++) {
            const int kb = kh2 * 9 + i, kk = kb >> 1, kh = kk / 3, kw = kk - kh * 3;
            const int khs = kh + rot >= 3 ? kh + rot - 3 : kh + rot;
            const int off = (khs * CF_NCOL + 2 * m + kw) * CF_COLB + ((kb & 1) * 16 + half * 8) * 2;   // col index = (2m+kw-1)+1
            const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(yh + off);
            const bf16x8 al = *reinterpret_cast<const bf16x8 *>(yl + off);
            if (NP == 3) {
                const bf16x8 am = *reinterpret_cast<const bf16x8 *>(ym + off);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bwm[i], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bwl[i], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bwh[i], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bwm[i], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bwh[i], acc, 0, 0, 0);
            } else {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bwl[i], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bwh[i], acc, 0, 0, 0);
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bwh[i], acc, 0, 0, 0);
        }
        // ---- reduce the two K halves, BN + ReLU, transpose to the output row through LDS
        if (kh2 == 1) {
#pragma unroll
            for (int r = 0; r < 16; r++) red[mt * 1024 + r * 64 + lane] = acc[r];
        }
        __syncthreads();
        if (kh2 == 0) {
            const float s1 = sc1[li], h1 = sh1[li];                                 // C/D: col = lane&31 = co
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int wo = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;         // row = w'
                if (wo < W2) {
                    float v = (acc[r] + red[mt * 1024 + r * 64 + lane]) * s1 + h1;
                    v = v > 0.f ? v : 0.f;
                    __bf16 hb = (__bf16)v;
                    const float r1 = v - (float)hb;
                    oh[li * W2 + wo] = *reinterpret_cast<unsigned short *>(&hb);
                    if (NP == 3) {
                        __bf16 mb = (__bf16)r1, lb = (__bf16)(r1 - (float)mb);
                        om[li * W2 + wo] = *reinterpret_cast<unsigned short *>(&mb);
                        ol[li * W2 + wo] = *reinterpret_cast<unsigned short *>(&lb);
                    } else { __bf16 lb = (__bf16)r1; ol[li * W2 + wo] = *reinterpret_cast<unsigned short *>(&lb); }
                }
            }
        }
        __syncthreads();
        // ---- row store.  NP = 3: 16-byte chunk q of a plane row = columns 8q .. 8q+7 = K-tile q / 4, offset (q % 4) * 8 of the tile-major
        // plane (out_hi = hi plane; mid and lo follow at plane strides of rows_total * 1952 elements, passed in out_lo as the mid plane)
        if (NP == 3) {
            const size_t mrows = (size_t)Tp * B;
            if (tid < 244) {
                const size_t dst = (((size_t)(tid >> 2) * mrows + rowid) * 32 + (tid & 3) * 8);
                *reinterpret_cast<u32x4 *>(out_hi + dst) = *reinterpret_cast<const u32x4 *>(oh + tid * 8);
                *reinterpret_cast<u32x4 *>(out_lo + dst) = *reinterpret_cast<const u32x4 *>(om + tid * 8);
                *reinterpret_cast<u32x4 *>(out_lo + mrows * ROW + dst) = *reinterpret_cast<const u32x4 *>(ol + tid * 8);
            }
            if (out_f32)
                for (int i = tid; i < ROW; i += 256)
                    out_f32[(size_t)rowid * ROW + i] = (__uint_as_float((unsigned)oh[i] << 16) + __uint_as_float((unsigned)om[i] << 16)) + __uint_as_float((unsigned)ol[i] << 16);
        } else {
            const size_t base = (size_t)rowid * ROW;
            if (tid < 244) *reinterpret_cast<u32x4 *>(out_hi + base + tid * 8) = *reinterpret_cast<const u32x4 *>(oh + tid * 8);
            else if (tid - 244 < 12) {   // 12 threads left in this pass: start the lo plane
                const int q = tid - 244;
                *reinterpret_cast<u32x4 *>(out_lo + base + q * 8) = *reinterpret_cast<const u32x4 *>(ol + q * 8);
            }
            if (tid < 232) {
                const int q = tid + 12;
                *reinterpret_cast<u32x4 *>(out_lo + base + q * 8) = *reinterpret_cast<const u32x4 *>(ol + q * 8);
            }
            if (out_f32)
                for (int i = tid; i < ROW; i += 256)
                    out_f32[base + i] = __uint_as_float((unsigned)oh[i] << 16) + __uint_as_float((unsigned)ol[i] << 16);
        }
    }
}

size_t conv_fused_smem(int np) { return 5 * CF_XLD * 4 + (size_t)np * CF_YPLANE + 2048 * 4 + (size_t)np * 1952 * 2; }

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
// LDS (R = 2): conv0 tile 3 planes x [5 slots][124 cols][64 B] (32 channels bf16; the four 16-byte chunks of a column are XOR-swizzled
// by column bits 2..3: 2-way-conflict fragment reads, as the padded layout of the row-wise kernel) | x tile [7][248] f32, whose bytes
// later stage the output rows [R][3 planes][1952] | K-half partial sums [2R tiles][16][64] f32 | conv0's folded BN (kept out of
// registers: with it there the kernel spills).
constexpr int CM_R = 2, CM_NY = 2 * CM_R + 1, CM_NX = 2 * CM_R + 3;
constexpr int CM_YPLANE = CM_NY * CF_NCOL * 64;                                    // 39680 B
constexpr int CM_XT = CM_NX * CF_XLD * 4, CM_OST = CM_R * 3 * 1952 * 2;             // 6944 B, 23424 B
constexpr int CM_RED = 2 * CM_R * 16 * 64 * 4;                                      // 16384 B: K-half partial sums of the 2R output tiles
constexpr size_t conv_multirow_smem() { return 3 * (size_t)CM_YPLANE + (CM_XT > CM_OST ? CM_XT : CM_OST) + CM_RED + 256; }   // 159104 B

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
            d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0m, bm, d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0h, bl, d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0l, bh, d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0h, bm, d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0m, bh, d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0h, bh, d, 0, 0, 0);
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
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bwm[i], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bwl[i], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bwh[i], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bwm[i], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bwh[i], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bwh[i], acc, 0, 0, 0);
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

int launch_conv_fused(const float *x, const float *w0, const float *sc0, const float *sh0, SplitPtr w1, const float *sc1,
                      const float *sh1, SplitPtr out, float *out_f32, int B, int T, int Traw, hipStream_t st) {
    // segments of consecutive output rows per utterance: about 1024 workgroups (two rounds of the 512 that fit the chip)
    const int Tp = T / 2;
    if (Tp <= 0 || B <= 0) return MDD_OK;
    int S = (1024 + B - 1) / B;
    S = S < 1 ? 1 : (S > Tp ? Tp : S);
    const int seg = (Tp + S - 1) / S;
    S = (Tp + seg - 1) / seg;                                                      // no empty segments
    hipLaunchKernelGGL(conv_fused_kernel<2>, dim3(B * S), dim3(256), conv_fused_smem(2), st, x, w0, sc0, sh0, w1.hi, w1.lo, sc1, sh1,
                       out.hi, out.lo, out_f32, B, T, Traw, S, seg);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// f32x6 form: w1_3 = conv1 weights [co][kh][kw][ci] as three consecutive row-major planes (hi | mid | lo, 32 * 288 elements each);
// out3 = three consecutive K-tile-major planes of (T/2 * B) x 1952 elements (the A operand of launch_gemm_f32x6)
// rowwise: the row-at-a-time kernel (MDD_CONV=rowwise, diagnostic); otherwise conv_fused_kernel<3, CM_R>, bit-identical to it.
int launch_conv_fused3(const float *x, const float *w0, const float *sc0, const float *sh0, const unsigned short *w1_3, const float *sc1,
                       const float *sh1, unsigned short *out3, float *out_f32, int B, int T, int Traw, hipStream_t st, bool rowwise,
                       long long *stamps) {
    const int Tp = T / 2;
    if (Tp <= 0 || B <= 0) return MDD_OK;
    int S = (512 + B - 1) / B;                                                     // one workgroup per CU (114 / 159 KB of LDS): two rounds of 256
    S = S < 1 ? 1 : (S > Tp ? Tp : S);
    int seg = (Tp + S - 1) / S;
    if (!rowwise) {
        seg = (seg + CM_R - 1) / CM_R * CM_R;                                      // whole blocks of CM_R rows except at the utterance's end
        S = (Tp + seg - 1) / seg;
        if (stamps) hipLaunchKernelGGL((conv_fused_kernel<3, CM_R, true>), dim3(B * S), dim3(512), conv_multirow_smem(), st, x, w0, sc0, sh0, w1_3,
                                       sc1, sh1, out3, out_f32, B, T, Traw, S, seg, stamps);
        else hipLaunchKernelGGL((conv_fused_kernel<3, CM_R, false>), dim3(B * S), dim3(512), conv_multirow_smem(), st, x, w0, sc0, sh0, w1_3,
                                sc1, sh1, out3, out_f32, B, T, Traw, S, seg, nullptr);
        MDD_LAUNCH_CHECK();
        return MDD_OK;
    }
    S = (Tp + seg - 1) / seg;
    const size_t plane = (size_t)Tp * B * 1952;
    hipLaunchKernelGGL(conv_fused_kernel<3>, dim3(B * S), dim3(256), conv_fused_smem(3), st, x, w0, sc0, sh0, w1_3, w1_3 + 32 * 288, sc1, sh1,
                       out3, out3 + plane, out_f32, B, T, Traw, S, seg);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

int init_conv_attributes() {
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)conv_fused_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)conv_fused_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)conv_fused_kernel<3, CM_R, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)conv_multirow_smem()));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)conv_fused_kernel<3, CM_R, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)conv_multirow_smem()));
    return MDD_OK;
}

}  // namespace mdd
