// The classifier tail of the CTC-only model (mdd_create_ctc).
//
// Reference: CRC/models/cnn_rnn.py:168-172, fc = BatchNorm1d(2H) + Linear(2H -> C, no bias), then LogSoftmax:
//   logp[r, :] = log_softmax( (X[r, :] * fscale + fshift) . Wfc^T )       r = t * B + b over the T' * B rows of the last BiLSTM layer's raw output
// Row-local: a row of logp depends on its own row of X and on the weights, nothing else.  No workgroup (and no wave) waits for another;
// neither kernel has a barrier.  All arithmetic is fp32 in every mode, as the attention tail's classifier (attn.hip) is.
//
// Floors: R * 2H * 4 bytes read, R * C * 4 written, 2 * R * 2H * C flop; at R = 128 k, H = 384 about 0.4 GB and 8.8 GFLOP, so the kernel
// is bound by the read of X (the classifier weights, 48 * 2H * 4 = 147 KB, stay in every L2).
#include "mdd_internal.h"

namespace mdd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- matrix-core form (2H % 64 == 0 and C <= 48: mfma_ctc_tail, plan.h) on v_mfma_f32_16x16x4_f32.
// A wave owns whole 16-row tiles of X over the full K = 2H, the four waves of a workgroup four neighbouring tiles.  Per 16 columns of K
// (group j) lane (li = lane & 15, kq = lane >> 4) holds, 16 bytes each,
//   A: y[r0 + li][16 j + 4 kq + m] = X * fscale + fshift, read straight from X;
//   B: wfcp[nt][j][lane][m] = Wfc[nt * 16 + li][16 j + 4 kq + m], repacked at finalize into this order (zero rows for n >= C);
// and MFMA number m of the group contracts the four k = 16 j + 4 kq + m, kq = 0 .. 3.  The three 16-column tiles accumulate in registers,
// in two levels as the attention tail does (64 k per segment, then one addition per segment).  D: row = 4 kq + i, col = li, so a row's
// C logits lie in the 16 lanes of one kq and the log-softmax is a reduction over those lanes.
__global__ __launch_bounds__(256) void ctc_tail_mfma_kernel(const float *__restrict__ X, const float *__restrict__ fscale, const float *__restrict__ fshift,
                                                            const float *__restrict__ wfcp, float *__restrict__ logp, int R, int K, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int tile = blockIdx.x * 4 + wave;
    if (tile * 16 >= R) return;
    const int r0 = tile * 16;
    const int J = K / 16;                                   // (J % 4 == 0: the launcher takes this kernel where K % 64 == 0)
    const int xrow = min(r0 + li, R - 1);                  // a last partial tile reads its last row again; those results are not stored
    const float *xsrc = X + (size_t)xrow * K + 4 * kq;     // + 16 j
    const float *scp = fscale + 4 * kq, *shp = fshift + 4 * kq;
    const float4 *wp = reinterpret_cast<const float4 *>(wfcp) + lane;   // + (nt * J + j) * 64

    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, t0 = a0, t1 = a0, t2 = a0;
    for (int j0 = 0; j0 < J; j0 += 4) {
        float4 y4[4], w0[4], w1[4], w2[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + u;
            w0[u] = wp[(0 * J + j) * 64]; w1[u] = wp[(1 * J + j) * 64]; w2[u] = wp[(2 * J + j) * 64];
            const float4 xv = *reinterpret_cast<const float4 *>(xsrc + 16 * j);
            const float4 sc = *reinterpret_cast<const float4 *>(scp + 16 * j), sh = *reinterpret_cast<const float4 *>(shp + 16 * j);
            y4[u] = make_float4(xv.x * sc.x + sh.x, xv.y * sc.y + sh.y, xv.z * sc.z + sh.z, xv.w * sc.w + sh.w);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(y4[u].x, w0[u].x, a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(y4[u].x, w1[u].x, a1, 0, 0, 0);
            a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(y4[u].x, w2[u].x, a2, 0, 0, 0);
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(y4[u].y, w0[u].y, a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(y4[u].y, w1[u].y, a1, 0, 0, 0);
            a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(y4[u].y, w2[u].y, a2, 0, 0, 0);
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(y4[u].z, w0[u].z, a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(y4[u].z, w1[u].z, a1, 0, 0, 0);
            a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(y4[u].z, w2[u].z, a2, 0, 0, 0);
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(y4[u].w, w0[u].w, a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(y4[u].w, w1[u].w, a1, 0, 0, 0);
            a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(y4[u].w, w2[u].w, a2, 0, 0, 0);
        }
        t0 += a0; t1 += a1; t2 += a2;
        a0 = (f32x4){0.f, 0.f, 0.f, 0.f}; a1 = a0; a2 = a0;
    }

    // log-softmax over C from the accumulators: row 4 kq + i of the tile lies in register i of the 16 lanes of this kq
    const bool c0 = li < C, c1 = 16 + li < C, c2 = 32 + li < C;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float v0 = c0 ? t0[i] : -INFINITY, v1 = c1 ? t1[i] : -INFINITY, v2 = c2 ? t2[i] : -INFINITY;
        float mx = fmaxf(fmaxf(v0, v1), v2);
        for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        float sum = (c0 ? expf(v0 - mx) : 0.f) + (c1 ? expf(v1 - mx) : 0.f) + (c2 ? expf(v2 - mx) : 0.f);
        for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        const float lse = logf(sum);
        const int r = r0 + 4 * kq + i;
        if (r < R) {
            float *orow = logp + (size_t)r * C;
            if (c0) orow[li] = (v0 - mx) - lse;
            if (c1) orow[16 + li] = (v1 - mx) - lse;
            if (c2) orow[32 + li] = (v2 - mx) - lse;
        }
    }
}

// ---- scalar form (every other accepted geometry): a wave per row, lanes over k.  A lane keeps its own y values (k = 4 lane + 256 i) in
// LDS, reading back only what it wrote itself; a logit is a wave reduction, left in the output row by lane c % 64, which also turns its
// own logits into log-probabilities once the row's maximum and sum are known.  K % 4 == 0 (hidden is a multiple of 4); any C.
// dynamic LDS: y[4 waves][K]
__global__ __launch_bounds__(256) void ctc_tail_kernel(const float *__restrict__ X, const float *__restrict__ fscale, const float *__restrict__ fshift,
                                                       const float *__restrict__ wfc, float *__restrict__ logp, int R, int K, int C) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave;
    if (r >= R) return;
    float *y = smem + (size_t)wave * K;
    const float *xr = X + (size_t)r * K;
    for (int k = lane * 4; k < K; k += 256) {
        const float4 xv = *reinterpret_cast<const float4 *>(xr + k);
        const float4 sc = *reinterpret_cast<const float4 *>(fscale + k), sh = *reinterpret_cast<const float4 *>(fshift + k);
        *reinterpret_cast<float4 *>(y + k) = make_float4(xv.x * sc.x + sh.x, xv.y * sc.y + sh.y, xv.z * sc.z + sh.z, xv.w * sc.w + sh.w);
    }
    float *orow = logp + (size_t)r * C;
    float mx = -INFINITY;   // of this lane's own logits
    for (int c = 0; c < C; c++) {
        const float *wr = wfc + (size_t)c * K;
        float acc = 0.f;
        for (int k = lane * 4; k < K; k += 256) {
            const float4 w4 = *reinterpret_cast<const float4 *>(wr + k);
            const float4 y4 = *reinterpret_cast<const float4 *>(y + k);
            acc = fmaf(w4.x, y4.x, acc); acc = fmaf(w4.y, y4.y, acc);
            acc = fmaf(w4.z, y4.z, acc); acc = fmaf(w4.w, y4.w, acc);
        }
        for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s);
        if ((c & 63) == lane) { orow[c] = acc; mx = fmaxf(mx, acc); }
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += expf(orow[c] - mx);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float lse = logf(sum);
    for (int c = lane; c < C; c += 64) orow[c] = (orow[c] - mx) - lse;
}

int launch_ctc_tail(const float *X, const float *fscale, const float *fshift, const float *wfc, const float *wfcp, float *logp, int R, int K, int C,
                    hipStream_t st) {
    if (R <= 0 || K <= 0 || K % 4 || C < 1 || (uintptr_t)X % 16) { set_error("ctc_tail: R=%d K=%d C=%d (K a multiple of 4, 16-byte aligned rows)", R, K, C); return MDD_ERR_ARG; }
    if (wfcp && K % 64 == 0 && C <= 48) {
        const int tiles = (R + 15) / 16;
        hipLaunchKernelGGL(ctc_tail_mfma_kernel, dim3((tiles + 3) / 4), dim3(256), 0, st, X, fscale, fshift, wfcp, logp, R, K, C);
        MDD_LAUNCH_CHECK();
        return MDD_OK;
    }
    const size_t smem = sizeof(float) * 4 * (size_t)K;   // at most 32 KB (hidden <= 1024)
    if (smem > 64 * 1024) { set_error("ctc_tail: 2H=%d too wide for the LDS rows (%zu B)", K, smem); return MDD_ERR_ARG; }
    hipLaunchKernelGGL(ctc_tail_kernel, dim3((R + 3) / 4), dim3(256), smem, st, X, fscale, fshift, wfc, logp, R, K, C);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

}  // namespace mdd
