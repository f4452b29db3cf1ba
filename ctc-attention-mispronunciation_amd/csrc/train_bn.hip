// Training step, train-mode BatchNorm over rows: column statistics, forward, backward, parameter gradients; column sums (layouts: train.h).
#include "train.h"

namespace mdd {

// ------------------------------------------------------------------------------------------------ BatchNorm over rows (train mode)
// Row-major x [R, F]; feature f is normalised over the R rows (BatchNorm2d on channels-last conv rows, BatchNorm1d on the
// [T'*B, F] rows of a sequence buffer: model_ctc.py:41-43, 153).  Column sums in fp64.
// mode 0: v = x                      (forward statistics)
// mode 1: dy = g (plain)             sums of dy and dy * xhat            (BatchNorm backward)
// mode 2: dy = g * mask * scale * (bn(x) > 0)   the same behind ReLU + dropout (LayerCNN: conv -> BN -> ReLU -> Dropout)
__device__ __forceinline__ float bn_site_dy(const BnSite &s, float g, float x, float mean, float invstd, float gamma, float beta, size_t row, int f, int F) {
    const float y = (x - mean) * invstd * gamma + beta;
    const float m = s.mask ? (float)s.mask[row * F + f] * s.scale : 1.f;
    return y > 0.f ? g * m : 0.f;
}
// dropout mask of a conv site, [B][F][T*W] (the reference's tensor order) -> [B][T*W][F] (the order of the channels-last rows)
__global__ __launch_bounds__(256) void mask_rows_kernel(const unsigned char *__restrict__ src, unsigned char *__restrict__ dst, int F, int TW) {
    __shared__ unsigned char tile[32][33];
    const size_t base = (size_t)blockIdx.z * F * TW;
    const int p0 = blockIdx.x * 32, f0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8) {
        const int f = f0 + j, p_ = p0 + tx;
        tile[j][tx] = (f < F && p_ < TW) ? src[base + (size_t)f * TW + p_] : 0;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int p_ = p0 + j, f = f0 + tx;
        if (p_ < TW && f < F) dst[base + (size_t)p_ * F + f] = tile[tx][j];
    }
}
int launch_mask_rows(const unsigned char *src, unsigned char *dst, int B, int F, int TW, hipStream_t st) {
    hipLaunchKernelGGL(mask_rows_kernel, dim3((TW + 31) / 32, (F + 31) / 32, B), dim3(256), 0, st, src, dst, F, TW);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}
template <int MODE>
__global__ __launch_bounds__(256) void col_stats_kernel(const float *__restrict__ x, const float *__restrict__ g, size_t R, int F, int rows_per_wg,
                                                        const float *__restrict__ mean, const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                        const float *__restrict__ beta, BnSite site, double *__restrict__ s1, double *__restrict__ s2) {
    __shared__ float p1[4][64], p2[4][64];
    const int tid = threadIdx.x, cl = tid & 63, rl = tid >> 6;
    const int f = blockIdx.x * 64 + cl;
    const size_t r0 = (size_t)blockIdx.y * rows_per_wg;
    float a1 = 0.f, a2 = 0.f;
    if (f < F) {
        float mu = 0.f, is = 0.f, ga = 1.f, be = 0.f;
        if (MODE != 0) { mu = mean[f]; is = invstd[f]; }
        if (MODE == 2) { ga = gamma[f]; be = beta[f]; }
        for (size_t r = r0 + rl; r < r0 + rows_per_wg && r < R; r += 4) {
            const float xv = x[r * F + f];
            if (MODE == 0) { a1 += xv; a2 = fmaf(xv, xv, a2); }
            else {
                const float dy = MODE == 1 ? g[r * F + f] : bn_site_dy(site, g[r * F + f], xv, mu, is, ga, be, r, f, F);
                a1 += dy; a2 = fmaf(dy, (xv - mu) * is, a2);
            }
        }
    }
    p1[rl][cl] = a1; p2[rl][cl] = a2;
    __syncthreads();
    if (tid < 64 && f < F) {
        atomicAdd(&s1[f], (double)p1[0][tid] + (double)p1[1][tid] + (double)p1[2][tid] + (double)p1[3][tid]);
        atomicAdd(&s2[f], (double)p2[0][tid] + (double)p2[1][tid] + (double)p2[2][tid] + (double)p2[3][tid]);
    }
}
// F = 32 (the conv sites: 2e7 elements in 6e5 rows): a lane owns four channels of a row (one 16-byte load), eight lanes a row, a
// wave eight rows per load instruction (1 KB, contiguous); partial sums per lane in fp32 over <= 32 rows, then fp64.
template <int MODE>
__global__ __launch_bounds__(256) void col_stats32_kernel(const float *__restrict__ x, const float *__restrict__ g, size_t R, int rows_per_wg,
                                                          const float *__restrict__ mean, const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, BnSite site, double *__restrict__ s1, double *__restrict__ s2) {
    constexpr int F = 32;
    __shared__ float q1[4][F], q2[4][F];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c4 = (lane & 7) * 4, rsub = lane >> 3;
    const size_t r0 = (size_t)blockIdx.x * rows_per_wg, r1 = min(r0 + (size_t)rows_per_wg, R);
    float a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f};
    float mu[4] = {0.f, 0.f, 0.f, 0.f}, is[4] = {0.f, 0.f, 0.f, 0.f}, ga[4] = {1.f, 1.f, 1.f, 1.f}, be[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (MODE != 0) { mu[j] = mean[c4 + j]; is[j] = invstd[c4 + j]; }
        if (MODE == 2) { ga[j] = gamma[c4 + j]; be[j] = beta[c4 + j]; }
    }
    for (size_t r = r0 + wave * 8 + rsub; r < r1; r += 32) {
        const float4 xq = *reinterpret_cast<const float4 *>(x + r * F + c4);
        const float xv[4] = {xq.x, xq.y, xq.z, xq.w};
        if (MODE == 0) {
#pragma unroll
            for (int j = 0; j < 4; j++) { a1[j] += xv[j]; a2[j] = fmaf(xv[j], xv[j], a2[j]); }
        } else {
            const float4 gq = *reinterpret_cast<const float4 *>(g + r * F + c4);
            const float gv[4] = {gq.x, gq.y, gq.z, gq.w};
            uchar4 mq = make_uchar4(1, 1, 1, 1);
            if (MODE == 2 && site.mask) mq = *reinterpret_cast<const uchar4 *>(site.mask + r * F + c4);
            const unsigned char mv[4] = {mq.x, mq.y, mq.z, mq.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float dy = gv[j];
                if (MODE == 2) {
                    const float y = (xv[j] - mu[j]) * is[j] * ga[j] + be[j];
                    const float m = site.mask ? (float)mv[j] * site.scale : 1.f;
                    dy = y > 0.f ? gv[j] * m : 0.f;
                }
                a1[j] += dy; a2[j] = fmaf(dy, (xv[j] - mu[j]) * is[j], a2[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) { a1[j] += __shfl_xor(a1[j], o); a2[j] += __shfl_xor(a2[j], o); }
    if (lane < 8) {
#pragma unroll
        for (int j = 0; j < 4; j++) { q1[wave][c4 + j] = a1[j]; q2[wave][c4 + j] = a2[j]; }
    }
    __syncthreads();
    if (tid < F) {
        atomicAdd(&s1[tid], ((double)q1[0][tid] + (double)q1[1][tid]) + ((double)q1[2][tid] + (double)q1[3][tid]));
        atomicAdd(&s2[tid], ((double)q2[0][tid] + (double)q2[1][tid]) + ((double)q2[2][tid] + (double)q2[3][tid]));
    }
}
template <int MODE>
static void launch_col_stats(const float *x, const float *g, size_t R, int F, const float *mean, const float *invstd, const float *gamma, const float *beta,
                             const BnSite &site, double *s1, double *s2, hipStream_t st) {
    if (F == 32 && (((size_t)x | (size_t)g) & 15) == 0) {
        const int per = 1024;
        hipLaunchKernelGGL(col_stats32_kernel<MODE>, dim3((unsigned)((R + per - 1) / per)), dim3(256), 0, st, x, g, R, per, mean, invstd, gamma, beta, site, s1, s2);
        return;
    }
    int per = (int)std::max<size_t>(64, (R + 255) / 256);
    dim3 grid((F + 63) / 64, (unsigned)((R + per - 1) / per));
    hipLaunchKernelGGL(col_stats_kernel<MODE>, grid, dim3(256), 0, st, x, g, R, F, per, mean, invstd, gamma, beta, site, s1, s2);
}
// mean / biased variance -> invstd; running statistics as nn.BatchNorm does (momentum 0.1, unbiased variance)
__global__ void bn_finalize_kernel(const double *s1, const double *s2, size_t R, int F, float eps, float momentum, float *mean, float *invstd,
                                   float *running_mean, float *running_var) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const double m = s1[f] / (double)R;
    double var = s2[f] / (double)R - m * m;
    if (var < 0) var = 0;
    mean[f] = (float)m;
    invstd[f] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
        const double unb = R > 1 ? var * (double)R / (double)(R - 1) : var;
        running_mean[f] = (1.f - momentum) * running_mean[f] + momentum * (float)m;
        running_var[f] = (1.f - momentum) * running_var[f] + momentum * (float)unb;
    }
}
// y = bn(x) [-> relu -> dropout]
// Elementwise BatchNorm kernels: the launch picks a grid whose stride (in elements) is a multiple of F, so a thread meets the same V
// features in every iteration and keeps their parameters in registers (bn_grid()).
template <int POST, int V>      // V = 4: F a multiple of 4 and 16-byte aligned buffers: four features of a row per thread
__global__ void bn_fwd_kernel(const float *__restrict__ x, size_t R, int F, const float *__restrict__ mean, const float *__restrict__ invstd,
                              const float *__restrict__ gamma, const float *__restrict__ beta, BnSite site, float *__restrict__ y) {
    const size_t n = R * F / V, q0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int f = (int)((q0 * V) % F);
    float mu[V], is[V], ga[V], be[V];
#pragma unroll
    for (int j = 0; j < V; j++) { mu[j] = mean[f + j]; is[j] = invstd[f + j]; ga[j] = gamma[f + j]; be[j] = beta[f + j]; }
    for (size_t q = q0; q < n; q += (size_t)gridDim.x * blockDim.x) {
        const size_t i = q * V;
        float xv[V], ov[V];
        unsigned char mv[V];
        if (V == 4) {
            const float4 t = *reinterpret_cast<const float4 *>(x + i); xv[0] = t.x; xv[1 % V] = t.y; xv[2 % V] = t.z; xv[3 % V] = t.w;
            if (POST && site.mask) { const uchar4 m = *reinterpret_cast<const uchar4 *>(site.mask + i); mv[0] = m.x; mv[1 % V] = m.y; mv[2 % V] = m.z; mv[3 % V] = m.w; }
        } else {
            xv[0] = x[i];
            if (POST && site.mask) mv[0] = site.mask[i];
        }
#pragma unroll
        for (int j = 0; j < V; j++) {
            float v = (xv[j] - mu[j]) * is[j] * ga[j] + be[j];
            if (POST) {
                const float m = site.mask ? (float)mv[j] * site.scale : 1.f;
                v = v > 0.f ? v * m : 0.f;
            }
            ov[j] = v;
        }
        if (V == 4) *reinterpret_cast<float4 *>(y + i) = make_float4(ov[0], ov[1 % V], ov[2 % V], ov[3 % V]);
        else y[i] = ov[0];
    }
}
// dx = gamma * invstd * (dy - sum(dy)/R - xhat * sum(dy*xhat)/R);  dgamma = sum(dy*xhat), dbeta = sum(dy)
template <int MODE, int V>
__global__ void bn_bwd_kernel(const float *__restrict__ x, const float *__restrict__ g, size_t R, int F, const float *__restrict__ mean,
                              const float *__restrict__ invstd, const float *__restrict__ gamma, const float *__restrict__ beta, BnSite site,
                              const double *__restrict__ s1, const double *__restrict__ s2, float *__restrict__ dx) {
    const size_t n = R * F / V, q0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int f = (int)((q0 * V) % F);
    float mu[V], is[V], ga[V], be[V], m1[V], m2[V];
#pragma unroll
    for (int j = 0; j < V; j++) {
        mu[j] = mean[f + j]; is[j] = invstd[f + j]; ga[j] = gamma[f + j]; be[j] = MODE == 2 ? beta[f + j] : 0.f;
        m1[j] = (float)(s1[f + j] / (double)R); m2[j] = (float)(s2[f + j] / (double)R);
    }
    for (size_t q = q0; q < n; q += (size_t)gridDim.x * blockDim.x) {
        const size_t i = q * V;
        float xv[V], gv[V], ov[V];
        unsigned char mv[V];
        if (V == 4) {
            const float4 t = *reinterpret_cast<const float4 *>(x + i); xv[0] = t.x; xv[1 % V] = t.y; xv[2 % V] = t.z; xv[3 % V] = t.w;
            const float4 u = *reinterpret_cast<const float4 *>(g + i); gv[0] = u.x; gv[1 % V] = u.y; gv[2 % V] = u.z; gv[3 % V] = u.w;
            if (MODE == 2 && site.mask) { const uchar4 m = *reinterpret_cast<const uchar4 *>(site.mask + i); mv[0] = m.x; mv[1 % V] = m.y; mv[2 % V] = m.z; mv[3 % V] = m.w; }
        } else {
            xv[0] = x[i]; gv[0] = g[i];
            if (MODE == 2 && site.mask) mv[0] = site.mask[i];
        }
#pragma unroll
        for (int j = 0; j < V; j++) {
            float dy = gv[j];
            if (MODE == 2) {   // behind ReLU + dropout (bn_site_dy's arithmetic)
                const float yv = (xv[j] - mu[j]) * is[j] * ga[j] + be[j];
                const float m = site.mask ? (float)mv[j] * site.scale : 1.f;
                dy = yv > 0.f ? gv[j] * m : 0.f;
            }
            const float xh = (xv[j] - mu[j]) * is[j];
            ov[j] = ga[j] * is[j] * (dy - m1[j] - xh * m2[j]);
        }
        if (V == 4) *reinterpret_cast<float4 *>(dx + i) = make_float4(ov[0], ov[1 % V], ov[2 % V], ov[3 % V]);
        else dx[i] = ov[0];
    }
}
// workgroups of 256 threads such that the grid's stride in elements (grid * 256 * V) is a multiple of F
static unsigned bn_grid(int F, int V) {
    int a = F, b = 256 * V;
    while (b) { const int t_ = a % b; a = b; b = t_; }              // a = gcd(F, 256 * V)
    const int unit = F / a;                                         // the grid must be a multiple of this
    return (unsigned)std::max(unit, 4096 / unit * unit);
}
__global__ void bn_param_grads_kernel(const double *s1, const double *s2, int F, float *dgamma, float *dbeta) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < F) { dgamma[f] = (float)s2[f]; dbeta[f] = (float)s1[f]; }
}

int launch_bn_train_fwd(const float *x, size_t R, int F, const float *gamma, const float *beta, float eps, float momentum, float *running_mean,
                        float *running_var, double *s1s2, float *mean, float *invstd, const BnSite *site, float *y, hipStream_t st) {
    MDD_HIP_CHECK(hipMemsetAsync(s1s2, 0, sizeof(double) * 2 * F, st));
    BnSite none{nullptr, 1.f};
    launch_col_stats<0>(x, nullptr, R, F, nullptr, nullptr, nullptr, nullptr, none, s1s2, s1s2 + F, st);
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((F + 127) / 128), dim3(128), 0, st, s1s2, s1s2 + F, R, F, eps, momentum, mean, invstd, running_mean, running_var);
    const bool v4 = F % 4 == 0 && (((size_t)x | (size_t)y) & 15) == 0 && (!site || !site->mask || ((size_t)site->mask & 3) == 0);
    if (site && v4) hipLaunchKernelGGL((bn_fwd_kernel<1, 4>), dim3(bn_grid(F, 4)), dim3(256), 0, st, x, R, F, mean, invstd, gamma, beta, *site, y);
    else if (site) hipLaunchKernelGGL((bn_fwd_kernel<1, 1>), dim3(bn_grid(F, 1)), dim3(256), 0, st, x, R, F, mean, invstd, gamma, beta, *site, y);
    else if (v4) hipLaunchKernelGGL((bn_fwd_kernel<0, 4>), dim3(bn_grid(F, 4)), dim3(256), 0, st, x, R, F, mean, invstd, gamma, beta, none, y);
    else hipLaunchKernelGGL((bn_fwd_kernel<0, 1>), dim3(bn_grid(F, 1)), dim3(256), 0, st, x, R, F, mean, invstd, gamma, beta, none, y);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}
int launch_bn_train_bwd(const float *x, const float *g, size_t R, int F, const float *gamma, const float *beta, const float *mean, const float *invstd,
                        const BnSite *site, double *s1s2, float *dx, float *dgamma, float *dbeta, hipStream_t st) {
    MDD_HIP_CHECK(hipMemsetAsync(s1s2, 0, sizeof(double) * 2 * F, st));
    BnSite none{nullptr, 1.f};
    const bool v4 = F % 4 == 0 && (((size_t)x | (size_t)g | (size_t)dx) & 15) == 0 && (!site || !site->mask || ((size_t)site->mask & 3) == 0);
    if (site) {
        launch_col_stats<2>(x, g, R, F, mean, invstd, gamma, beta, *site, s1s2, s1s2 + F, st);
        if (v4) hipLaunchKernelGGL((bn_bwd_kernel<2, 4>), dim3(bn_grid(F, 4)), dim3(256), 0, st, x, g, R, F, mean, invstd, gamma, beta, *site, s1s2, s1s2 + F, dx);
        else hipLaunchKernelGGL((bn_bwd_kernel<2, 1>), dim3(bn_grid(F, 1)), dim3(256), 0, st, x, g, R, F, mean, invstd, gamma, beta, *site, s1s2, s1s2 + F, dx);
    } else {
        launch_col_stats<1>(x, g, R, F, mean, invstd, gamma, beta, none, s1s2, s1s2 + F, st);
        if (v4) hipLaunchKernelGGL((bn_bwd_kernel<1, 4>), dim3(bn_grid(F, 4)), dim3(256), 0, st, x, g, R, F, mean, invstd, gamma, beta, none, s1s2, s1s2 + F, dx);
        else hipLaunchKernelGGL((bn_bwd_kernel<1, 1>), dim3(bn_grid(F, 1)), dim3(256), 0, st, x, g, R, F, mean, invstd, gamma, beta, none, s1s2, s1s2 + F, dx);
    }
    hipLaunchKernelGGL(bn_param_grads_kernel, dim3((F + 127) / 128), dim3(128), 0, st, s1s2, s1s2 + F, F, dgamma, dbeta);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}
__global__ void col_sum_finish_kernel(const double *s1, int F, float *out) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < F) out[f] = (float)s1[f];
}
// column sums of g [R, F] -> out[F] (bias gradients)
int launch_col_sum(const float *g, size_t R, int F, double *s1s2, float *out, hipStream_t st) {
    MDD_HIP_CHECK(hipMemsetAsync(s1s2, 0, sizeof(double) * 2 * F, st));
    BnSite none{nullptr, 1.f};
    launch_col_stats<0>(g, nullptr, R, F, nullptr, nullptr, nullptr, nullptr, none, s1s2, s1s2 + F, st);
    hipLaunchKernelGGL(col_sum_finish_kernel, dim3((F + 127) / 128), dim3(128), 0, st, s1s2, F, out);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

}  // namespace mdd
