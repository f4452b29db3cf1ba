// Training step, row and element kernels: dropout, column copies, softmax rows, the embedding gradient, partial-sum reduce, Adam (layouts: train.h).
#include "train.h"

namespace mdd {

// ------------------------------------------------------------------------------------------------ dropout masks
// counter-based generator: mask[i] = hash(seed, site, i) keeps with probability 1 - p
__global__ void dropout_mask_kernel(unsigned char *mask, size_t n, unsigned long long seed, unsigned site, float p) {
    const unsigned thresh = (unsigned)((double)p * 4294967296.0);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (i + 1) + ((unsigned long long)site << 56);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        mask[i] = (unsigned)(z >> 32) >= thresh ? 1 : 0;
    }
}
int launch_dropout_mask(unsigned char *mask, size_t n, unsigned long long seed, unsigned site, float p, hipStream_t st) {
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st, mask, n, seed, site, p);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// ------------------------------------------------------------------------------------------------ elementwise helpers
// y = x * mask * scale (mask in the same [rows, F] order); in place allowed
__global__ void dropout_rows_kernel(const float *__restrict__ x, const unsigned char *__restrict__ mask, float scale, size_t n, float *__restrict__ y) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = mask ? x[i] * ((float)mask[i] * scale) : x[i];
}
int launch_dropout_rows(const float *x, const unsigned char *mask, float scale, size_t n, float *y, hipStream_t st) {
    hipLaunchKernelGGL(dropout_rows_kernel, dim3(4096), dim3(256), 0, st, x, mask, scale, n, y);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}
// dst[r, c0 + j] (ld_dst) (+)= src[r, s0 + j] (ld_src), j < width
__global__ void copy_cols_kernel(const float *__restrict__ src, int ld_src, int s0, float *__restrict__ dst, int ld_dst, int c0, size_t R, int width, int add) {
    const size_t n = R * width;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / width; const int j = (int)(i % width);
        const float v = src[r * ld_src + s0 + j];
        float *d = dst + r * ld_dst + c0 + j;
        *d = add ? *d + v : v;
    }
}
int launch_copy_cols(const float *src, int ld_src, int s0, float *dst, int ld_dst, int c0, size_t R, int width, bool add, hipStream_t st) {
    hipLaunchKernelGGL(copy_cols_kernel, dim3(4096), dim3(256), 0, st, src, ld_src, s0, dst, ld_dst, c0, R, width, add ? 1 : 0);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}
// rows of length n: y = softmax(x) or log_softmax(x) (one wave per row)
template <int LOG>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float *__restrict__ x, size_t R, int n, float *__restrict__ y) {
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const float *xr = x + r * n;
    float m = -INFINITY;
    for (int j = lane; j < n; j += 64) m = fmaxf(m, xr[j]);
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float s = 0.f;
    for (int j = lane; j < n; j += 64) s += expf(xr[j] - m);
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    const float ls = logf(s);
    for (int j = lane; j < n; j += 64) y[r * n + j] = LOG ? (xr[j] - m) - ls : expf(xr[j] - m) / s;
}
int launch_softmax_rows(const float *x, size_t R, int n, float *y, bool log, hipStream_t st) {
    dim3 grid((unsigned)((R + 3) / 4)), block(256);
    if (log) hipLaunchKernelGGL(softmax_rows_kernel<1>, grid, block, 0, st, x, R, n, y);
    else hipLaunchKernelGGL(softmax_rows_kernel<0>, grid, block, 0, st, x, R, n, y);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}
// LOG: dx = g - exp(y) * sum(g)   (y = log-probs);   else: dx = y * (g - sum(g * y))   (y = probabilities)
template <int LOG>
__global__ __launch_bounds__(256) void softmax_bwd_rows_kernel(const float *__restrict__ y, const float *__restrict__ g, size_t R, int n, float *__restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    float s = 0.f;
    for (int j = lane; j < n; j += 64) s += LOG ? g[r * n + j] : g[r * n + j] * y[r * n + j];
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    for (int j = lane; j < n; j += 64) {
        const float yv = y[r * n + j], gv = g[r * n + j];
        dx[r * n + j] = LOG ? gv - expf(yv) * s : yv * (gv - s);
    }
}
int launch_softmax_bwd_rows(const float *y, const float *g, size_t R, int n, float *dx, bool log, hipStream_t st) {
    dim3 grid((unsigned)((R + 3) / 4)), block(256);
    if (log) hipLaunchKernelGGL(softmax_bwd_rows_kernel<1>, grid, block, 0, st, y, g, R, n, dx);
    else hipLaunchKernelGGL(softmax_bwd_rows_kernel<0>, grid, block, 0, st, y, g, R, n, dx);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}
// dE[v, :] = sum over positions m = l*B + b with ids[b, l] == v of g[m, :]   (ascending m: deterministic)
__global__ __launch_bounds__(128) void embed_bwd_kernel(const float *__restrict__ g, const int64_t *__restrict__ ids, int B, int L, int E, float *__restrict__ dE) {
    __shared__ int sid[1024];                                       // the ids of 1024 positions at a time: only the matching ones touch g
    const int v = blockIdx.x, e = blockIdx.y * blockDim.x + threadIdx.x, LB = L * B;
    float acc = 0.f;
    for (int m0 = 0; m0 < LB; m0 += 1024) {
        const int nm = min(1024, LB - m0);
        for (int j = threadIdx.x; j < nm; j += blockDim.x) { const int m = m0 + j, l = m / B, b = m - l * B; sid[j] = (int)ids[(size_t)b * L + l]; }
        __syncthreads();
        if (e < E)
            for (int j = 0; j < nm; j++)
                if (sid[j] == v) acc += g[(size_t)(m0 + j) * E + e];
        __syncthreads();
    }
    if (e < E) dE[(size_t)v * E + e] = acc;
}
int launch_embed_bwd(const float *g, const int64_t *ids, int B, int L, int E, int rows, float *dE, hipStream_t st) {
    hipLaunchKernelGGL(embed_bwd_kernel, dim3(rows, (E + 127) / 128), dim3(128), 0, st, g, ids, B, L, E, dE);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}
// sum of `parts` partial matrices of n elements (split-K GEMM outputs): out[i] = sum_z part[z*n + i]
__global__ void reduce_parts_kernel(const float *__restrict__ part, int parts, size_t n, float *__restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        double acc = 0.0;
        for (int z = 0; z < parts; z++) acc += (double)part[(size_t)z * n + i];
        out[i] = (float)acc;
    }
}
int launch_reduce_parts(const float *part, int parts, size_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(reduce_parts_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, st, part, parts, n, out);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}

// ------------------------------------------------------------------------------------------------ Adam (torch.optim.Adam semantics, L2 weight decay)
// g' = g + wd * p;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// The betas arrive as doubles and everything that depends on them alone is formed in double on the host and rounded ONCE, as torch does
// (1 - beta2 reaches ATen as the double 0.001 and becomes 0.001f): 1.f - 0.999f is 0.0009999871, -1.29e-5 relative, which exp_avg_sq carried.
struct AdamCoef { float b1, b2, omb1, omb2, bc1, bc2_sqrt; };       // beta, 1 - beta, 1 - beta1^step, sqrt(1 - beta2^step)
static AdamCoef adam_coef(double b1, double b2, int step) {
    return {(float)b1, (float)b2, (float)(1.0 - b1), (float)(1.0 - b2), (float)(1.0 - std::pow(b1, (double)step)), (float)std::sqrt(1.0 - std::pow(b2, (double)step))};
}
__global__ void adam_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, size_t n, float lr, AdamCoef c,
                            float eps, float wd) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float gi = g[i] + wd * p[i];
        const float mi = c.b1 * m[i] + c.omb1 * gi;
        const float vi = c.b2 * v[i] + c.omb2 * gi * gi;
        m[i] = mi; v[i] = vi;
        p[i] -= (lr / c.bc1) * (mi / (sqrtf(vi) / c.bc2_sqrt + eps));
    }
}
int launch_adam(float *p, const float *g, float *m, float *v, size_t n, float lr, double b1, double b2, float eps, float wd, int step, hipStream_t st) {
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, st, p, g, m, v, n, lr, adam_coef(b1, b2, step), eps, wd);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// The same update over up to 48 tensors in ONE launch (the reference model has 43 parameter tensors -- and 12 buffers, which Adam never sees --, most of them small: one launch each was a
// quarter millisecond of launches per step).  The table travels in the kernel arguments; workgroup w works on 1024-element chunk
// w - first[t] of tensor t (first[] = running chunk counts).
constexpr int ADAM_MT = 48;
struct AdamTable { float *p[ADAM_MT]; const float *g[ADAM_MT]; float *m[ADAM_MT]; float *v[ADAM_MT]; unsigned long long n[ADAM_MT]; int first[ADAM_MT + 1]; int count; };
__global__ __launch_bounds__(256) void adam_multi_kernel(AdamTable tb, float lr, AdamCoef c, float eps, float wd) {
    int t = 0;
    while (t + 1 < tb.count && (int)blockIdx.x >= tb.first[t + 1]) t++;            // (uniform per workgroup; <= 48 steps)
    const size_t i0 = (size_t)((int)blockIdx.x - tb.first[t]) * 1024;
    float *p = tb.p[t], *m = tb.m[t], *v = tb.v[t];
    const float *g = tb.g[t];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t i = i0 + threadIdx.x + 256 * k;
        if (i < tb.n[t]) {
            const float gi = g[i] + wd * p[i];
            const float mi = c.b1 * m[i] + c.omb1 * gi;
            const float vi = c.b2 * v[i] + c.omb2 * gi * gi;
            m[i] = mi; v[i] = vi;
            p[i] -= (lr / c.bc1) * (mi / (sqrtf(vi) / c.bc2_sqrt + eps));
        }
    }
}
int launch_adam_multi(float *const *p, float *const *g, float *const *m, float *const *v, const int64_t *numel, int n, float lr, double b1, double b2, float eps,
                      float wd, int step, hipStream_t st) {
    const AdamCoef coef = adam_coef(b1, b2, step);
    int i = 0;
    while (i < n) {
        AdamTable tb;
        tb.count = 0; tb.first[0] = 0;
        for (; i < n && tb.count < ADAM_MT; i++) {
            if (!p[i] || !g[i] || numel[i] <= 0) continue;
            const int c = tb.count++;
            tb.p[c] = p[i]; tb.g[c] = g[i]; tb.m[c] = m[i]; tb.v[c] = v[i]; tb.n[c] = (unsigned long long)numel[i];
            tb.first[c + 1] = tb.first[c] + (int)((numel[i] + 1023) / 1024);
        }
        if (tb.count == 0) break;
        hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)tb.first[tb.count]), dim3(256), 0, st, tb, lr, coef, eps, wd);
        MDD_LAUNCH_CHECK();
    }
    return MDD_OK;
}

}  // namespace mdd
