// Operand preparation for the bf16 matrix-core GEMMs: every kernel that turns fp32 values into bf16 planes (bf16_split.h has the arithmetic).
//   two planes (gemm_bf16x3.hip), row-major:   launch_split / launch_unsplit (flat), launch_split_rows / launch_transpose_split (a matrix as
//                                              it stands or transposed, the contraction zero-padded)
//   three planes (gemm_bf16x6.hip), K-tile-major: launch_split3 / launch_split3_pad (rows), launch_transpose_split3 (stored [K, rows])
//   three planes, row-major: launch_split3_rowmajor (the conv1 weights of the conv timing aid)
#include "bf16_split.h"
#include "mdd_internal.h"

namespace mdd {

// fp32 [n] -> hi/lo planes (used for weights at load time and by the tap / test helpers)
__global__ void split_kernel(const float *__restrict__ x, size_t n, unsigned short *__restrict__ hi, unsigned short *__restrict__ lo) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = x[i];
        const unsigned short h = bf16_bits(v);
        hi[i] = h;
        lo[i] = bf16_bits(v - bf16_to_f32(h));
    }
}
__global__ void unsplit_kernel(const unsigned short *__restrict__ hi, const unsigned short *__restrict__ lo, size_t n, float *__restrict__ x) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        x[i] = bf16_to_f32(hi[i]) + bf16_to_f32(lo[i]);
}

int launch_split(const float *x, size_t n, const SplitPtr &out, hipStream_t st) {
    int grid = (int)((n + 255) / 256); if (grid > 4096) grid = 4096; if (grid < 1) grid = 1;
    hipLaunchKernelGGL(split_kernel, dim3(grid), dim3(256), 0, st, x, n, out.hi, out.lo);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}
int launch_unsplit(const SplitPtr &in, size_t n, float *x, hipStream_t st) {
    int grid = (int)((n + 255) / 256); if (grid > 4096) grid = 4096; if (grid < 1) grid = 1;
    hipLaunchKernelGGL(unsplit_kernel, dim3(grid), dim3(256), 0, st, in.hi, in.lo, n, x);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// ---- the operands of the training step's split-bf16 contractions (gemm_bf16x3_ops).  The planes of an fp32 matrix as it stands (rows x
// cols, the contraction along the columns, zero-padded to cols_pad) or transposed (the contraction along the ROWS: out[c][r] = src[r][c],
// zero-padded to rows_pad), which turns the NN and TN products of the backward pass into the NT form.
__global__ void split_rows_kernel(const float *__restrict__ src, int ld, size_t rows, int cols, int cols_pad, unsigned short *__restrict__ hi,
                                  unsigned short *__restrict__ lo) {
    const size_t n = rows * cols_pad;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / cols_pad; const int c = (int)(i % cols_pad);
        split_store(c < cols ? src[r * ld + c] : 0.f, hi, lo, i);
    }
}
__global__ __launch_bounds__(256) void transpose_split_kernel(const float *__restrict__ src, int ld, int rows, int cols, int rows_pad,
                                                              unsigned short *__restrict__ hi, unsigned short *__restrict__ lo) {
    __shared__ float tile[32][33];
    const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8 threads
    for (int j = ty; j < 32; j += 8) {
        const int r = r0 + j, c = c0 + tx;
        tile[j][tx] = (r < rows && c < cols) ? src[(size_t)r * ld + c] : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, r = r0 + tx;
        if (c < cols && r < rows_pad) split_store(tile[tx][j], hi, lo, (size_t)c * rows_pad + r);
    }
}
int launch_split_rows(const float *src, int ld, size_t rows, int cols, int cols_pad, unsigned short *hi, unsigned short *lo, hipStream_t st) {
    hipLaunchKernelGGL(split_rows_kernel, dim3(4096), dim3(256), 0, st, src, ld, rows, cols, cols_pad, hi, lo);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}
int launch_transpose_split(const float *src, int ld, int rows, int cols, int rows_pad, unsigned short *hi, unsigned short *lo, hipStream_t st) {
    hipLaunchKernelGGL(transpose_split_kernel, dim3((rows_pad + 31) / 32, (cols + 31) / 32), dim3(256), 0, st, src, ld, rows, cols, rows_pad, hi, lo);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}

// ---- three planes (hi, mid, lo) for the f32x6 kernel, each in the K-TILE-MAJOR order it streams: plane[kt][row][32] (kt = k / 32), so that
// the 16 rows x 64 bytes one LDS-DMA instruction moves are 1 KB of CONTIGUOUS memory (eight whole 128-byte lines, every byte used).  With
// row-major planes the same instruction touched 16 half-lines, and the kernel ran at the rate a CU ingests lines from L2 (~25 useful B/clk).
// Both kernels write planes of `rows` x Kp elements, plane_elems apart, with the contraction axis zero-padded from K to Kp (a multiple of
// 32): a padded position is zero in all three planes, so a padded K-tile adds exact zeros to every accumulator.
//
// The row operand, x [rows][ld] with K leading columns used (any K).  One wave per (16-row group, K-tile): lane (row = lane / 4, chunk =
// lane % 4) reads 8 floats, writes 16 bytes per plane; a lane whose eight columns reach past K reads what is there one float at a time and
// zeros for the rest.  This kernel defines the layout and the arithmetic that the other producers of such planes follow (lstm_x6.hip,
// the fused conv front end).
__global__ void split3_pad_kernel(const float *__restrict__ x, int rows, int K, int ld, int Kp, unsigned short *__restrict__ planes, size_t plane_elems) {
    const int lane = threadIdx.x & 63;
    const int nkt = Kp / 32, ngr = (rows + 15) / 16;
    const size_t total = (size_t)ngr * nkt;
    for (size_t w = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < total; w += (size_t)gridDim.x * (blockDim.x >> 6)) {
        const int g = (int)(w / nkt), kt = (int)(w - (size_t)g * nkt);
        const int row = g * 16 + (lane >> 2), c = lane & 3, k0 = kt * 32 + c * 8;
        if (row >= rows) continue;
        const float *src = x + (size_t)row * ld + k0;
        float f[8];
        if (k0 + 8 <= K) {
            const float4 v0 = reinterpret_cast<const float4 *>(src)[0], v1 = reinterpret_cast<const float4 *>(src)[1];
            f[0] = v0.x; f[1] = v0.y; f[2] = v0.z; f[3] = v0.w; f[4] = v1.x; f[5] = v1.y; f[6] = v1.z; f[7] = v1.w;
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) f[k] = k0 + k < K ? src[k] : 0.f;
        }
        split3_store8(f, planes, plane_elems, ((size_t)kt * rows + row) * 32 + c * 8);
    }
}

// The transposed operand: x is stored [K][ld] with `rows` leading columns used, and the operand's row r is x's COLUMN r (the contraction runs
// down x's rows).  One workgroup per (K-tile, 64 operand rows): the 32 x 64 block is read along x's rows (16 lanes x 16 bytes = 256 contiguous
// bytes per x row), turned in LDS, and leaves as 64 rows x 64 bytes per plane = 4 KB of contiguous memory, 16 bytes per lane.
// LDS row pitch 33 words: the turn's writes (bank 4 m4 + k) and its reads (bank r + 8 c + j) both spread over the banks.
constexpr int TS3_R = 64;
__global__ __launch_bounds__(256) void transpose_split3_kernel(const float *__restrict__ x, int K, int rows, int ld, unsigned short *__restrict__ planes,
                                                               size_t plane_elems) {
    __shared__ float tile[TS3_R][33];
    const int kt = blockIdx.x, r0 = blockIdx.y * TS3_R, tid = threadIdx.x;
    {
        const int m4 = tid & 15, rr = r0 + m4 * 4;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int kl = (tid >> 4) + h * 16, k = kt * 32 + kl;
            float4 v = {0.f, 0.f, 0.f, 0.f};
            if (k < K) {
                const float *src = x + (size_t)k * ld + rr;
                if (rr + 3 < rows) v = *reinterpret_cast<const float4 *>(src);
                else { if (rr < rows) v.x = src[0]; if (rr + 1 < rows) v.y = src[1]; if (rr + 2 < rows) v.z = src[2]; }
            }
            tile[m4 * 4 + 0][kl] = v.x; tile[m4 * 4 + 1][kl] = v.y; tile[m4 * 4 + 2][kl] = v.z; tile[m4 * 4 + 3][kl] = v.w;
        }
    }
    __syncthreads();
    const int rl = tid >> 2, c = tid & 3, row = r0 + rl;
    if (row >= rows) return;
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; k++) f[k] = tile[rl][c * 8 + k];
    split3_store8(f, planes, plane_elems, ((size_t)kt * rows + row) * 32 + c * 8);
}

static bool split3_args_ok(const float *x, int rows, int K, int ld, int Kp, const unsigned short *planes, size_t plane_elems) {
    return x && planes && rows > 0 && K > 0 && Kp >= K && Kp % 32 == 0 && ld % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)planes % 16 == 0 &&
           plane_elems % 8 == 0 && plane_elems >= (size_t)rows * Kp;
}
int launch_split3_pad(const float *x, int rows, int K, int ld, int Kp, unsigned short *planes, size_t plane_elems, hipStream_t st) {
    if (!split3_args_ok(x, rows, K, ld, Kp, planes, plane_elems) || ld < K) {
        set_error("split3_pad: rows=%d K=%d ld=%d Kp=%d (Kp a multiple of 32 >= K, ld a multiple of 4 >= K, 16-byte aligned)", rows, K, ld, Kp); return MDD_ERR_ARG;
    }
    const size_t waves = (size_t)((rows + 15) / 16) * (Kp / 32);
    int grid = (int)((waves + 3) / 4); if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL(split3_pad_kernel, dim3(grid), dim3(256), 0, st, x, rows, K, ld, Kp, planes, plane_elems);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}
// The unpadded form (the decode path's operands and weights): K a multiple of 32, three consecutive planes of rows x K elements.
int launch_split3(const float *x, int rows, int K, int ld, unsigned short *planes, hipStream_t st) {
    if (rows <= 0 || K <= 0 || K % 32 || ld % 4) { set_error("split3: rows=%d K=%d ld=%d (K a multiple of 32, ld of 4)", rows, K, ld); return MDD_ERR_ARG; }
    return launch_split3_pad(x, rows, K, ld, K, planes, (size_t)rows * K, st);
}
int launch_transpose_split3(const float *x, int K, int rows, int ld, int Kp, unsigned short *planes, size_t plane_elems, hipStream_t st) {
    if (!split3_args_ok(x, rows, K, ld, Kp, planes, plane_elems) || ld < rows || (rows + TS3_R - 1) / TS3_R > 65535) {
        set_error("transpose_split3: K=%d rows=%d ld=%d Kp=%d (Kp a multiple of 32 >= K, ld a multiple of 4 >= rows, 16-byte aligned)", K, rows, ld, Kp); return MDD_ERR_ARG;
    }
    hipLaunchKernelGGL(transpose_split3_kernel, dim3(Kp / 32, (rows + TS3_R - 1) / TS3_R), dim3(256), 0, st, x, K, rows, ld, planes, plane_elems);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// row-major hi | mid | lo planes of n elements each (the fused conv front end's conv1 weights)
__global__ void split3_rowmajor_kernel(const float *w, int n, unsigned short *planes) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        unsigned short h, m, l;
        split3(w[i], h, m, l);
        planes[i] = h; planes[n + i] = m; planes[2 * n + i] = l;
    }
}
int launch_split3_rowmajor(const float *w, int n, unsigned short *planes, hipStream_t st) {
    hipLaunchKernelGGL(split3_rowmajor_kernel, dim3((n + 255) / 256), dim3(256), 0, st, w, n, planes);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

}  // namespace mdd
