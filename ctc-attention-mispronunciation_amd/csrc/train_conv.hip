// Training step, CNN: conv0 forward and weight gradient, the im2col path of conv1, W1 packing, the CNN <-> sequence relayout (layouts: train.h).
// conv1's direct kernels: train_conv1.hip.
#include "train.h"

namespace mdd {

// ------------------------------------------------------------------------------------------------ conv0 (1 -> ch), direct
// z0[(b,t,w), c] = bias[c] + sum_{kh,kw} x[b, t+kh-1, 2w+kw-1] * w0[c, kh, kw]      (Conv2d k3x3, stride (1,2), pad 1)
template <int CH>
__global__ __launch_bounds__(256) void conv0_train_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
                                                              float *__restrict__ z, int B, int T, int F, int W1) {
    const size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x, npos = (size_t)B * T * W1;
    if (pos >= npos) return;
    const int wo = (int)(pos % W1), t = (int)((pos / W1) % T), b = (int)(pos / ((size_t)W1 * T));
    float in[9];
#pragma unroll
    for (int kh = 0; kh < 3; kh++)
#pragma unroll
        for (int kw = 0; kw < 3; kw++) {
            const int ti = t + kh - 1, fi = wo * 2 + kw - 1;
            in[kh * 3 + kw] = (ti >= 0 && ti < T && fi >= 0 && fi < F) ? x[((size_t)b * T + ti) * F + fi] : 0.f;
        }
    float *o = z + pos * CH;
#pragma unroll 4
    for (int c = 0; c < CH; c++) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 9; k++) acc = fmaf(in[k], w[c * 9 + k], acc);
        o[c] = acc + bias[c];
    }
}
int launch_conv0_train_fwd(const float *x, const float *w, const float *bias, float *z, int B, int T, int F, int ch, hipStream_t st) {
    const int W1 = (F + 2 - 3) / 2 + 1;
    const size_t npos = (size_t)B * T * W1;
    dim3 grid((unsigned)((npos + 255) / 256)), block(256);
    if (!with_conv_channels(ch, [&](auto c) { hipLaunchKernelGGL(conv0_train_fwd_kernel<decltype(c)::value>, grid, block, 0, st, x, w, bias, z, B, T, F, W1); }))
        { set_error("conv0 (train): channels=%d not built", ch); return MDD_ERR_ARG; }
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// dW0[c, k] = sum_pos dz0[pos, c] * patch[pos, k];  db0[c] = sum_pos dz0[pos, c].  Partial sums per workgroup in LDS (fp32), one
// fp64 atomic per (workgroup, entry): the order of the adds moves the result by ~1e-16 relative, far below fp32 rounding.
template <int CH>
__global__ __launch_bounds__(256) void conv0_train_bwd_kernel(const float *__restrict__ x, const float *__restrict__ dz, double *__restrict__ acc /*[CH*10]*/,
                                                              int B, int T, int F, int W1, int rows_per_wave) {
    // A wave walks whole (b, t) rows of W1 output positions.  lane = (position slot, channel): the CH lanes of a slot read one contiguous
    // dz row and the same nine input samples (broadcast); a lane keeps its channel's nine tap sums and the bias sum (k = 9) in registers
    // (rows_per_wave * W1 * CH / 64 terms in fp32), then fp64 across workgroups.
    constexpr int PPW = 64 / CH;
    __shared__ float part[4][CH * 10];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane % CH, slot = lane / CH;
    const int nrow = B * T, row0 = (blockIdx.x * 4 + wave) * rows_per_wave;
    float sum[10];
#pragma unroll
    for (int k = 0; k < 10; k++) sum[k] = 0.f;
    for (int row = row0; row < min(row0 + rows_per_wave, nrow); row++) {
        const int t = row % T;
        const float *xr = x + (size_t)row * F;                      // input row t of utterance b; rows t-1 / t+1 exist unless at the edge
        const bool up = t > 0, dn = t + 1 < T;
        const float *dzr = dz + (size_t)row * W1 * CH;
        for (int wo = slot; wo < W1; wo += PPW) {
            const float dzv = dzr[wo * CH + c];
#pragma unroll
            for (int kw = 0; kw < 3; kw++) {
                const int fi = wo * 2 + kw - 1;
                const bool in = fi >= 0 && fi < F;
                const float p0 = (in && up) ? xr[fi - F] : 0.f, p1 = in ? xr[fi] : 0.f, p2 = (in && dn) ? xr[fi + F] : 0.f;
                sum[kw] = fmaf(dzv, p0, sum[kw]); sum[3 + kw] = fmaf(dzv, p1, sum[3 + kw]); sum[6 + kw] = fmaf(dzv, p2, sum[6 + kw]);
            }
            sum[9] += dzv;
        }
    }
#pragma unroll
    for (int k = 0; k < 10; k++)
#pragma unroll
        for (int o = CH; o < 64; o <<= 1) sum[k] += __shfl_xor(sum[k], o);
    if (lane < CH) {
#pragma unroll
        for (int k = 0; k < 10; k++) part[wave][c * 10 + k] = sum[k];
    }
    __syncthreads();
    for (int e = tid; e < CH * 10; e += 256) atomicAdd(&acc[e], (double)((part[0][e] + part[1][e]) + (part[2][e] + part[3][e])));
}
__global__ void conv0_bwd_finish_kernel(const double *acc, float *dw, float *db, int ch) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ch * 10) return;
    const int c = e / 10, k = e - c * 10;
    if (k < 9) dw[c * 9 + k] = (float)acc[e]; else db[c] = (float)acc[e];
}
int launch_conv0_train_bwd(const float *x, const float *dz, double *acc, float *dw, float *db, int B, int T, int F, int ch, hipStream_t st) {
    const int W1 = (F + 2 - 3) / 2 + 1;
    MDD_HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(double) * ch * 10, st));
    const int rpw = 4;                                             // (b, t) rows per wave: ~500 workgroups at B*T = 8000
    dim3 grid((unsigned)((B * T + 4 * rpw - 1) / (4 * rpw))), block(256);
    if (!with_conv_channels(ch, [&](auto c) { hipLaunchKernelGGL(conv0_train_bwd_kernel<decltype(c)::value>, grid, block, 0, st, x, dz, acc, B, T, F, W1, rpw); }))
        { set_error("conv0 (train): channels=%d not built", ch); return MDD_ERR_ARG; }
    hipLaunchKernelGGL(conv0_bwd_finish_kernel, dim3((ch * 10 + 63) / 64), dim3(64), 0, st, acc, dw, db, ch);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// ------------------------------------------------------------------------------------------------ conv1 (ch -> ch, stride 2x2) as im2col + GEMM
// col[(b,t',w'), (kh*3+kw)*ch + ci] = a0[b, 2t'+kh-1, 2w'+kw-1, ci]   (zero outside)
__global__ void im2col1_kernel(const float *__restrict__ a0, float *__restrict__ col, int B, int T, int W1, int W2, int ch) {
    const int Tp = T / 2, Kc = 9 * ch, c4n = ch / 4;
    const size_t n = (size_t)B * Tp * W2 * 9 * c4n;    // one thread per 16 bytes of col, in col's own order: stores (and each tap's loads) are contiguous
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4n) * 4;
        const size_t pt = i / c4n;
        const int tap = (int)(pt % 9);
        const size_t pos = pt / 9;
        const int wo = (int)(pos % W2), tp = (int)((pos / W2) % Tp), b = (int)(pos / ((size_t)W2 * Tp));
        const int ti = 2 * tp + tap / 3 - 1, wi = 2 * wo + tap % 3 - 1;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ti >= 0 && ti < T && wi >= 0 && wi < W1) v = *reinterpret_cast<const float4 *>(a0 + (((size_t)b * T + ti) * W1 + wi) * ch + c);
        *reinterpret_cast<float4 *>(col + pos * Kc + tap * ch + c) = v;
    }
}
// da0[b,t,w,ci] = sum over the (<= 4) output positions / taps that read it of dcol
__global__ void col2im1_kernel(const float *__restrict__ dcol, float *__restrict__ da0, int B, int T, int W1, int W2, int ch) {
    const int Tp = T / 2, Kc = 9 * ch, c4n = ch / 4;
    const size_t n = (size_t)B * T * W1 * c4n;                      // four channels of an input position per thread (the taps' adds in the same order as before)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int ci = (int)(i % c4n) * 4;
        const size_t p = i / c4n;
        const int w = (int)(p % W1), t = (int)((p / W1) % T), b = (int)(p / ((size_t)W1 * T));
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int kh = 0; kh < 3; kh++) {
            const int tt = t + 1 - kh;
            if (tt < 0 || (tt & 1) || (tt >> 1) >= Tp) continue;
#pragma unroll
            for (int kw = 0; kw < 3; kw++) {
                const int ww = w + 1 - kw;
                if (ww < 0 || (ww & 1) || (ww >> 1) >= W2) continue;
                const float4 v = *reinterpret_cast<const float4 *>(dcol + (((size_t)b * Tp + (tt >> 1)) * W2 + (ww >> 1)) * Kc + (kh * 3 + kw) * ch + ci);
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
        }
        *reinterpret_cast<float4 *>(da0 + p * ch + ci) = acc;
    }
}
// W1 [co][ci][kh][kw] <-> W1r [co][(kh*3+kw)*ch + ci]
__global__ void pack_w1_kernel(const float *__restrict__ w, float *__restrict__ wr, int ch, int to_packed) {
    const int n = ch * ch * 9, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = i % 9, ci = (i / 9) % ch, co = i / (9 * ch);
    const int j = (co * 9 + k) * ch + ci;
    if (to_packed) wr[j] = w[i]; else wr[i] = w[j];     // unpack: wr is the reference-layout destination, w the packed source
}
int launch_im2col1(const float *a0, float *col, int B, int T, int W1, int W2, int ch, hipStream_t st) {
    hipLaunchKernelGGL(im2col1_kernel, dim3(4096), dim3(256), 0, st, a0, col, B, T, W1, W2, ch);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}
int launch_col2im1(const float *dcol, float *da0, int B, int T, int W1, int W2, int ch, hipStream_t st) {
    hipLaunchKernelGGL(col2im1_kernel, dim3(8192), dim3(256), 0, st, dcol, da0, B, T, W1, W2, ch);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}
int launch_pack_w1(const float *src, float *dst, int ch, bool to_packed, hipStream_t st) {
    hipLaunchKernelGGL(pack_w1_kernel, dim3((ch * ch * 9 + 255) / 256), dim3(256), 0, st, src, dst, ch, to_packed ? 1 : 0);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}

// a1 [B,T',W2,ch] (channels-last) <-> seq [T',B, c*W2 + w]   (model_ctc.py:176-181; feature index = c*W2 + w)
__global__ void cnn_seq_kernel(float *__restrict__ a1, float *__restrict__ seq, int B, int Tp, int W2, int ch, int to_seq) {
    const size_t n = (size_t)B * Tp * W2 * ch;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % ch);
        const size_t p = i / ch;
        const int w = (int)(p % W2), t = (int)((p / W2) % Tp), b = (int)(p / ((size_t)W2 * Tp));
        const size_t j = ((size_t)t * B + b) * ((size_t)ch * W2) + (size_t)c * W2 + w;
        if (to_seq) seq[j] = a1[i]; else a1[i] = seq[j];
    }
}
int launch_cnn_seq(float *a1, float *seq, int B, int Tp, int W2, int ch, bool to_seq, hipStream_t st) {
    hipLaunchKernelGGL(cnn_seq_kernel, dim3(4096), dim3(256), 0, st, a1, seq, B, Tp, W2, ch, to_seq ? 1 : 0);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}

}  // namespace mdd
