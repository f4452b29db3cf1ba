// Split-bf16 ("bf16x3") NT GEMM on the gfx950 bf16 matrix cores: C[M,N] = A[M,K] . W[N,K]^T (+ bias).
//
// Every fp32 operand x is carried as two bf16 planes, hi = bf16(x) and lo = bf16(x - hi) (16 mantissa
// bits together), and the product is evaluated as  Ah.Wh + Ah.Wl + Al.Wh  with fp32 accumulation in
// v_mfma_f32_32x32x16_bf16.  The dropped Al.Wl term is 2^-16 of a product; measured on the whole model
// (4 x BiLSTM-384, T'=100) the log-probs move by 7.6e-6 against 1.9e-6 for the exact-fp32 MFMA path,
// both far inside the 1e-4 parity tolerance (DESIGN.md "precision modes").  Three bf16 MFMAs cost 3/16 of
// the fp32 MFMA they replace, which is why the time-batched contractions of the path run here:
// BiLSTM input projections (AA/models/model_ctc.py:28-29,44), text-encoder projection (:150,198),
// `score` Linear (:151,201) and the attention scores bmm (:204).
//
// Operands arrive pre-split from their producers (conv1, the LSTM step epilogue, the embedding gather;
// weights are split once at load time), so this kernel moves the same 4 bytes per element an fp32 GEMM
// would and spends no VALU on conversion.
//
// Kernels (all stream their operands HBM -> LDS with LDS-DMA, 16 B per lane, and use v_mfma_f32_16x16x32_bf16 with the WEIGHT
// fragment as the first operand, so that a lane's four accumulator registers are four consecutive C columns): the 8-phase 256x256
// kernel (large projections), the single-barrier 256x256 kernel it is screened against, and the 128x128 kernel (small / batched /
// split-output GEMMs).  An output element is accumulated identically in all of them (batch-size independent bits).  The
// register-staged and 32x32x16 forms of round 1 measured slower and are no longer built.
//
// This file holds the kernels and their launchers only: the operand planes are made in split.hip, the timing and screening entries that
// drive these launchers are in diag.hip.
#include "bf16_split.h"
#include "train.h"

namespace mdd {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int XBM = 128, XBN = 128, XBK = 32, XROW = 64;   // XROW: bytes per LDS row (32 bf16, unpadded, XOR-swizzled)
constexpr int XPLANE = XBM * XROW;                          // 8192 B
// LDS layout: 16-byte chunk c of row r lives at chunk position c ^ ((r >> 2) & 3): the ds_read_b128 fragment reads
// (16-lane groups {0-3,12-15,20-27}, ..: rows sharing r&3 differ in (r>>2)&3) and the ds_write_b128 staging writes are
// bank-conflict-free.
//
__device__ __forceinline__ bf16x8 x3_frag(const unsigned char *plane, int row, int kbyte) {
    return *reinterpret_cast<const bf16x8 *>(plane + row * XROW + ((((kbyte >> 4) ^ ((row >> 2) & 3))) << 4));
}

// ---- LDS-DMA variant of the 128x128 kernel: tiles go global -> LDS directly (global_load_lds_dwordx4), no staging
// registers and no ds_write pass.  The LDS image is lane-linear per wave-instruction (64 x 16 B = 16 rows of one plane),
// so the XOR swizzle is applied to the per-lane SOURCE address; fragment reads use the same swizzle (x3_frag).
typedef __attribute__((address_space(3))) void lds_void;

__device__ __forceinline__ void x3_glds_tile(const unsigned short *__restrict__ Ah, const unsigned short *__restrict__ Al,
                                             const unsigned short *__restrict__ Wh, const unsigned short *__restrict__ Wl, int lda, int ldw,
                                             int M, int N, int m0, int n0, int k0, unsigned char *stage, int wave, int lane) {
    // wave w issues 8 instructions: plane p = j>>1, 16-row group g = (j&1)*4 + w
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int p = j >> 1, g = (j & 1) * 4 + wave;
        const int row = g * 16 + (lane >> 2), cp = lane & 3, c = cp ^ ((row >> 2) & 3);
        const unsigned short *base = p == 0 ? Ah : (p == 1 ? Al : (p == 2 ? Wh : Wl));
        const int ld = p < 2 ? lda : ldw, rtot = p < 2 ? M : N, r0 = p < 2 ? m0 : n0;
        const unsigned short *src = base + (size_t)min(r0 + row, rtot - 1) * ld + k0 + c * 8;
        __builtin_amdgcn_global_load_lds(src, (lds_void *)(stage + p * XPLANE + g * 1024), 16, 0, 0);
    }
}

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_bf16x3_glds_kernel(const unsigned short *__restrict__ Ah, const unsigned short *__restrict__ Al,
                                                                   const unsigned short *__restrict__ Wh, const unsigned short *__restrict__ Wl,
                                                                   const float *__restrict__ bias, float *__restrict__ C,
                                                                   unsigned short *__restrict__ Ch, unsigned short *__restrict__ Cl, int M, int N,
                                                                   int K, int lda, int ldw, int ldc, long sA, long sW, long sC, int tiles_n, int pA, int pW) {
    // v_mfma_f32_16x16x32_bf16, per wave 64x64 = 4x4 tiles.  Same shape and product order as the 256x256 kernel, so an
    // output element is accumulated identically whichever kernel the problem size selects (results do not depend on
    // how many utterances share the batch, bit for bit).
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][4 * XPLANE];   // one array: [stage][Ah|Al|Wh|Wl]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    int nwg = gridDim.x, bid = blockIdx.x;
    int q = nwg >> 3, rem = nwg & 7, xcd = bid & 7;
    int swz = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (bid >> 3);
    const int tm = swz / tiles_n, tn = swz % tiles_n;
    const int m0 = tm * XBM, n0 = tn * XBN;
    // pA / pW (SplitOperand::period): product z reads matrix z % period of that operand
    const size_t za = pA ? blockIdx.z % pA : blockIdx.z, zw = pW ? blockIdx.z % pW : blockIdx.z;
    Ah += za * sA; Al += za * sA;
    Wh += zw * sW; Wl += zw * sW;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nk = K / XBK;
    const int l16 = lane & 15, kq16 = (lane >> 4) * 16;
    x3_glds_tile(Ah, Al, Wh, Wl, lda, ldw, M, N, m0, n0, 0, lds[0], wave, lane);
    __syncthreads();   // hipcc drains the LDS-DMA (vmcnt(0)) ahead of the barrier
    for (int kt = 0; kt < nk; kt++) {
        const int cur = kt & 1;
        if (kt + 1 < nk) x3_glds_tile(Ah, Al, Wh, Wl, lda, ldw, M, N, m0, n0, (kt + 1) * XBK, lds[cur ^ 1], wave, lane);
        const unsigned char *st = lds[cur];
        bf16x8 fwh[4], fwl[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            fwh[j] = x3_frag(st + 2 * XPLANE, wn * 64 + j * 16 + l16, kq16);
            fwl[j] = x3_frag(st + 3 * XPLANE, wn * 64 + j * 16 + l16, kq16);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const bf16x8 fah = x3_frag(st, wm * 64 + i * 16 + l16, kq16);
            const bf16x8 fal = x3_frag(st + XPLANE, wm * 64 + i * 16 + l16, kq16);
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fwl[j], fah, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fwh[j], fal, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fwh[j], fah, acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    const int q4 = (lane >> 4) * 4;   // W fragment first: D row = 4*(lane>>4) + r = C column, D col = lane&15 = C row
    if (EPI == 0) C += (size_t)blockIdx.z * sC; else { Ch += (size_t)blockIdx.z * sC; Cl += (size_t)blockIdx.z * sC; }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int row = m0 + wm * 64 + i * 16 + l16;
            if (row >= M) continue;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int col = n0 + wn * 64 + j * 16 + q4 + r;
                if (col >= N) continue;
                const float v = acc[i][j][r] + (bias ? bias[col] : 0.f);
                if (EPI == 0) C[(size_t)row * ldc + col] = v;
                else {
                    const unsigned short h = bf16_bits(v);
                    Ch[(size_t)row * ldc + col] = h;
                    Cl[(size_t)row * ldc + col] = bf16_bits(v - bf16_to_f32(h));
                }
            }
        }
}

// ---- LDS-DMA, 256x256 tile, 8 waves (2 x 4), per wave 128x64: half the L2 -> LDS bytes per flop of the 128x128 tile.
__global__ __launch_bounds__(512, 2) void gemm_bf16x3_glds256_kernel(const unsigned short *__restrict__ Ah, const unsigned short *__restrict__ Al,
                                                                      const unsigned short *__restrict__ Wh, const unsigned short *__restrict__ Wl,
                                                                      const float *__restrict__ bias, float *__restrict__ C, int M, int N, int K,
                                                                      int lda, int ldw, int ldc, int tiles_n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char glds_smem[];   // [2 stages][Ah|Al|Wh|Wl][256 rows x 64 B] = 128 KB
    constexpr int PL = 256 * XROW;                                              // 16 KB per plane
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    int nwg = gridDim.x, bid = blockIdx.x;
    int q = nwg >> 3, rem = nwg & 7, xcd = bid & 7;
    int swz = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (bid >> 3);
    const int tm = swz / tiles_n, tn = swz % tiles_n;
    const int m0 = tm * 256, n0 = tn * 256;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f32x4 acc16[8][4];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc16[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto fill = [&](int k0, unsigned char *stage, int j0 = 0, int j1 = 8) {
#pragma unroll
        for (int j = j0; j < j1; j++) {
            const int id = j * 8 + wave, p = id >> 4, g = id & 15;
            const int row = g * 16 + (lane >> 2), cp = lane & 3, c = cp ^ ((row >> 2) & 3);
            const unsigned short *base = p == 0 ? Ah : (p == 1 ? Al : (p == 2 ? Wh : Wl));
            const int ld = p < 2 ? lda : ldw, rtot = p < 2 ? M : N, r0 = p < 2 ? m0 : n0;
            const unsigned short *src = base + (size_t)min(r0 + row, rtot - 1) * ld + k0 + c * 8;
            __builtin_amdgcn_global_load_lds(src, (lds_void *)(stage + p * PL + g * 1024), 16, 0, 0);
        }
    };
    const int nk = K / XBK;
    fill(0, glds_smem);
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nk;
        unsigned char *nst = glds_smem + (cur ^ 1) * 4 * PL;
        const unsigned char *st = glds_smem + cur * 4 * PL;
        // v_mfma_f32_16x16x32_bf16: one k-step per K-tile; lane (row l&15, k-slice l>>4)
        const int l16 = lane & 15, kq16 = (lane >> 4) * 16;
        bf16x8 fwh[4], fwl[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            fwh[j] = x3_frag(st + 2 * PL, wn * 64 + j * 16 + l16, kq16);
            fwl[j] = x3_frag(st + 3 * PL, wn * 64 + j * 16 + l16, kq16);
        }
        // the next stage's 8 LDS-DMA pieces go out two at a time between the MFMA groups: a piece costs the issuing
        // wave 100+ cycles, which the SIMD's other wave covers with MFMAs only if the two are not doing it at once
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if ((i & 1) == 0) {
                if (more) fill((kt + 1) * XBK, nst, i, i + 2);
                __builtin_amdgcn_sched_barrier(0);
            }
            const bf16x8 fah = x3_frag(st, wm * 128 + i * 16 + l16, kq16);
            const bf16x8 fal = x3_frag(st + PL, wm * 128 + i * 16 + l16, kq16);
#pragma unroll
            for (int j = 0; j < 4; j++) acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fwl[j], fah, acc16[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; j++) acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fwh[j], fal, acc16[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; j++) acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fwh[j], fah, acc16[i][j], 0, 0, 0);
            if (i & 1) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    }
    {   // W fragment first: D row = 4*(lane>>4) + r = C column, D col = lane&15 = C row (see the 8-phase kernel)
        const int l16 = lane & 15, q4 = (lane >> 4) * 4;
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int row = m0 + wm * 128 + i * 16 + l16;
                if (row >= M) continue;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int col = n0 + wn * 64 + j * 16 + q4 + r;
                    if (col < N) C[(size_t)row * ldc + col] = acc16[i][j][r] + (bias ? bias[col] : 0.f);
                }
            }
    }
}

// ---- 256x256 tile, eight barrier-delimited phases per K-tile, two wave groups one barrier apart.
// Same LDS image and the same per-element arithmetic as gemm_bf16x3_glds256_kernel (identical bits); what changes is
// who waits for what.  The K-tile's operands are four half-tiles (A rows 0..127 / 128..255, W rows 0..127 / 128..255;
// hi + lo planes, 16 KB = 16 LDS-DMA pieces = 2 per wave) and a wave's share of C is four 64x32 quadrants (A half a,
// W half b) taken in the order (0,0) (0,1) (1,1) (1,0).  A quadrant is a load phase L (fragment reads for it, the two
// DMA pieces of one half-tile of the NEXT K-tile, a counted s_waitcnt vmcnt(4) that retires the half-tile the next L
// will read while the two issued after it stay in flight) and an MFMA phase M (24 MFMAs), each ended by a raw
// s_barrier.  Waves 4..7 (the other wave of every SIMD) run one barrier behind waves 0..3, so one group's M always
// overlaps the other group's L: the matrix pipe no longer idles while both waves of a SIMD read fragments and wait.
// Hazards: a half-tile issued in phase p is waited for at the end of L(p+2) by every wave, read in L(p+3) -- for the
// late group that is after one more barrier than the early group's wait, as the stagger requires -- and its buffer is
// refilled eight phases later.
template <bool STAMP>
__global__ __launch_bounds__(512, 2) void gemm_bf16x3_ph8_kernel(const unsigned short *__restrict__ Ah, const unsigned short *__restrict__ Al,
                                                                 const unsigned short *__restrict__ Wh, const unsigned short *__restrict__ Wl,
                                                                 const float *__restrict__ bias, float *__restrict__ C, int M, int N, int K,
                                                                 int lda, int ldw, int ldc, int tiles_n, long long *stamps = nullptr) {
    // STAMP (diagnostic build only): per wave, cycles spent in load-phase bodies / waiting at their barrier / MFMA-phase bodies /
    // waiting at theirs, summed over the K loop -> stamps[(workgroup * 8 + wave) * 4 + {0,1,2,3}]
    long long sacc[4] = {0, 0, 0, 0}, stt = 0;
#define PH8_T(i_) do { if (STAMP) { const long long n_ = (long long)__builtin_readcyclecounter(); sacc[i_] += n_ - stt; stt = n_; } } while (0)
    extern __shared__ __attribute__((aligned(16))) unsigned char glds_smem[];   // [2 stages][Ah|Al|Wh|Wl][256 rows x 64 B] = 128 KB
    constexpr int PL = 256 * XROW;                                              // 16 KB per plane
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wr = (wave >> 1) & 1, wc = (wave & 1) + 2 * grp;   // SIMD partners w, w+4 sit in different groups
    int nwg = gridDim.x, bid = blockIdx.x;
    int q = nwg >> 3, rem = nwg & 7, xcd = bid & 7;
    int swz = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (bid >> 3);
    const int tm = swz / tiles_n, tn = swz % tiles_n;
    const int m0 = tm * 256, n0 = tn * 256;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f32x4 acc[2][2][4][2];                                          // [A half][W half][row tile][col tile]
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[a][b][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // half-tile ht of the K-tile at k0 -> stage: 0 = A half 0, 1 = W half 0, 2 = W half 1, 3 = A half 1; this wave's 2 pieces.
    // Addresses are a wave-uniform base (SGPR pair, advanced by k0) plus a per-lane 32-bit byte offset fixed for the
    // whole K loop, and the LDS address is scalar too: no vector address arithmetic inside the loop (on this chip a
    // SIMD's vector instructions are not covered by its MFMAs).
    const unsigned wave_s = __builtin_amdgcn_readfirstlane((unsigned)wave);
    const unsigned lds0 = (unsigned)(unsigned long long)(lds_void *)glds_smem;
    unsigned voff[4];
#pragma unroll
    for (int ht = 0; ht < 4; ht++) {
        const bool isA = ht == 0 || ht == 3;
        const int half = (ht >= 2) ? 1 : 0, g = half * 8 + wave;     // 16-row group inside the plane
        const int row = g * 16 + (lane >> 2), cp = lane & 3, c = cp ^ ((row >> 2) & 3);
        const int ld = isA ? lda : ldw, rtot = isA ? M : N, r0 = isA ? m0 : n0;
        voff[ht] = (unsigned)(((size_t)min(r0 + row, rtot - 1) * ld + c * 8) * 2);
    }
    auto issue = [&](int ht, int k0, unsigned stage_off) {
        const bool isA = ht == 0 || ht == 3;
        const unsigned g = ((ht >= 2) ? 8u : 0u) + wave_s;
        const unsigned short *bh = (isA ? Ah : Wh) + k0, *bl = (isA ? Al : Wl) + k0;
        const unsigned la = lds0 + stage_off + g * 1024u;
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff[ht]), "s"(bh), "s"(la + (unsigned)((isA ? 0 : 2) * PL)) : "memory", "m0");
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff[ht]), "s"(bl), "s"(la + (unsigned)((isA ? 1 : 3) * PL)) : "memory", "m0");
    };
    const int nk = K / XBK;
    const int l16 = lane & 15, kq16 = (lane >> 4) * 16;
#pragma unroll
    for (int ht = 0; ht < 4; ht++) issue(ht, 0, 0u);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                 // A0, W0 of K-tile 0
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (grp == 1) asm volatile("s_barrier" ::: "memory");            // from here on one barrier behind group 0
    bf16x8 fah[4], fal[4], fwh[2][2], fwl[2][2];                     // A fragments of the current half; W fragments of both halves
#define PH8_END_L() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); PH8_T(0); asm volatile("s_barrier" ::: "memory"); PH8_T(1); __builtin_amdgcn_s_setprio(1)
#define PH8_END_M() __builtin_amdgcn_s_setprio(0); PH8_T(2); asm volatile("s_barrier" ::: "memory"); PH8_T(3)
#define PH8_LOAD_A(a_) _Pragma("unroll") for (int i = 0; i < 4; i++) { \
            fah[i] = x3_frag(st, (a_) * 128 + wr * 64 + i * 16 + l16, kq16); fal[i] = x3_frag(st + PL, (a_) * 128 + wr * 64 + i * 16 + l16, kq16); }
#define PH8_LOAD_W(b_) _Pragma("unroll") for (int j = 0; j < 2; j++) { \
            fwh[b_][j] = x3_frag(st + 2 * PL, (b_) * 128 + wc * 32 + j * 16 + l16, kq16); fwl[b_][j] = x3_frag(st + 3 * PL, (b_) * 128 + wc * 32 + j * 16 + l16, kq16); }
#define PH8_MFMA(a_, b_) _Pragma("unroll") for (int i = 0; i < 4; i++) { \
            _Pragma("unroll") for (int j = 0; j < 2; j++) acc[a_][b_][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fwl[b_][j], fah[i], acc[a_][b_][i][j], 0, 0, 0); \
            _Pragma("unroll") for (int j = 0; j < 2; j++) acc[a_][b_][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fwh[b_][j], fal[i], acc[a_][b_][i][j], 0, 0, 0); \
            _Pragma("unroll") for (int j = 0; j < 2; j++) acc[a_][b_][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fwh[b_][j], fah[i], acc[a_][b_][i][j], 0, 0, 0); }
    // The LDS-DMA pieces are issued from the load phases.  The form that issued the two pieces of a phase pair from inside the MFMA phase
    // (behind its first MFMA group; each counted wait then saw one issue less, vmcnt(2) for vmcnt(4)) lost and is no longer built.  Stamps
    // (profiles/round2_gemm_phase_stamps.txt): the MFMA phases, not the load phases, set the length of a barrier interval (per K-tile and
    // wave: MFMA bodies 1744 cycles against load bodies 1336), so moving issue work into them lengthens the interval: 5-8 % slower.
    if (STAMP) stt = (long long)__builtin_readcyclecounter();
    for (int kt = 0; kt < nk; kt++) {
        const unsigned char *st = glds_smem + (kt & 1) * 4 * PL;
        const unsigned nst = (unsigned)(((kt & 1) ^ 1) * 4 * PL);   // byte offset of the other stage
        const bool more = kt + 1 < nk;
        const int nk0 = (kt + 1) * XBK;
        // ---- quadrant (0,0)
        PH8_LOAD_A(0) PH8_LOAD_W(0)
        if (more) issue(0, nk0, nst);
        if (more) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");   // W1 of this K-tile
        __builtin_amdgcn_sched_barrier(0);
        PH8_END_L();
        PH8_MFMA(0, 0)
        __builtin_amdgcn_sched_barrier(0);
        PH8_END_M();
        // ---- quadrant (0,1)
        PH8_LOAD_W(1)
        if (more) issue(1, nk0, nst);
        if (more) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // A1 of this K-tile
        __builtin_amdgcn_sched_barrier(0);
        PH8_END_L();
        PH8_MFMA(0, 1)
        __builtin_amdgcn_sched_barrier(0);
        PH8_END_M();
        // ---- quadrant (1,1)
        PH8_LOAD_A(1)
        if (more) issue(2, nk0, nst);
        __builtin_amdgcn_sched_barrier(0);
        PH8_END_L();
        PH8_MFMA(1, 1)
        __builtin_amdgcn_sched_barrier(0);
        PH8_END_M();
        // ---- quadrant (1,0): its fragments are already in registers
        if (more) { issue(3, nk0, nst); asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); }                             // A0, W0 of the next K-tile
        __builtin_amdgcn_sched_barrier(0);
        PH8_END_L();
        PH8_MFMA(1, 0)
        __builtin_amdgcn_sched_barrier(0);
        PH8_END_M();
    }
    if (STAMP && stamps && lane == 0 && blockIdx.x < 256)
        for (int i = 0; i < 4; i++) stamps[((size_t)blockIdx.x * 8 + wave) * 4 + i] = sacc[i];
#undef PH8_T
#undef PH8_END_L
#undef PH8_END_M
#undef PH8_LOAD_A
#undef PH8_LOAD_W
#undef PH8_MFMA
    if (grp == 0) asm volatile("s_barrier" ::: "memory");            // pairs with group 1's last barrier
    // The W fragment is the MFMA's first operand (D rows = weight rows = C columns) and the A fragment its second (D columns = C
    // rows): D row = 4*(lane>>4) + r, D col = lane&15, so a lane's four accumulator registers are FOUR CONSECUTIVE COLUMNS of one C
    // row -- the tile leaves as 16-byte stores (32 per wave, 16 rows x 64 B each) instead of 128 scalar ones.
    const int q4 = (lane >> 4) * 4;
    const bool n_vec = (ldc % 4 == 0) && (((size_t)C & 15) == 0);
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int row = m0 + a * 128 + wr * 64 + i * 16 + l16;
                    const int col = n0 + b * 128 + wc * 32 + j * 16 + q4;
                    if (row >= M || col >= N) continue;
                    const f32x4 v = acc[a][b][i][j];
                    float *dst = C + (size_t)row * ldc + col;
                    if (n_vec && col + 3 < N) {
                        float4 o = make_float4(v[0], v[1], v[2], v[3]);
                        if (bias) { const float4 bv = *reinterpret_cast<const float4 *>(bias + col); o.x += bv.x; o.y += bv.y; o.z += bv.z; o.w += bv.w; }
                        *reinterpret_cast<float4 *>(dst) = o;
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; r++) if (col + r < N) dst[r] = v[r] + (bias ? bias[col + r] : 0.f);
                    }
                }
}


int init_gemm_attributes() {
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)gemm_bf16x3_glds256_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 4 * 256 * XROW));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)gemm_bf16x3_ph8_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 4 * 256 * XROW));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)gemm_bf16x3_ph8_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 4 * 256 * XROW));
    return MDD_OK;
}

static bool x3_args_ok(const SplitOperand &A, const SplitOperand &W, int M, int N, int K, int batch) {
    if (M > 0 && N > 0 && K > 0 && batch > 0 && K % XBK == 0 && A.ld % 8 == 0 && W.ld % 8 == 0 && A.stride % 8 == 0 && W.stride % 8 == 0) return true;
    set_error("gemm_bf16x3: bad shape M=%d N=%d K=%d lda=%d ldw=%d (K must be a multiple of %d)", M, N, K, A.ld, W.ld, XBK);
    return false;
}

// One of the 256x256-tile kernels on one product (no batch, fp32 output).  The 8-phase kernel is production's; the single-barrier kernel
// and the stamped instantiation run in the diagnostics only (stamps: nullable, the stamped form's phase cycle sums).
int launch_gemm_bf16x3_256(X3Form form, const SplitOperand &A, const SplitOperand &W, float *C, int ldc, int M, int N, int K, hipStream_t st,
                           const float *bias, long long *stamps) {
    if (!x3_args_ok(A, W, M, N, K, 1)) return MDD_ERR_ARG;
    if (A.period || W.period) { set_error("gemm_bf16x3_256: one product, no operand period (launch_gemm_bf16x3 runs it)"); return MDD_ERR_ARG; }
    const int tn = (N + 255) / 256;
    const dim3 grid(((M + 255) / 256) * tn), block(512);
    const size_t smem = 2 * 4 * 256 * XROW;
#define GO(kernel_, ...) hipLaunchKernelGGL(kernel_, grid, block, smem, st, A.p.hi, A.p.lo, W.p.hi, W.p.lo, bias, C, M, N, K, A.ld, W.ld, ldc, tn, ##__VA_ARGS__)
    if (form == X3Form::SingleBarrier) GO(gemm_bf16x3_glds256_kernel);
    else if (form == X3Form::Phase8) GO(gemm_bf16x3_ph8_kernel<false>, (long long *)nullptr);
    else GO(gemm_bf16x3_ph8_kernel<true>, stamps);
#undef GO
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

int launch_gemm_bf16x3(const SplitOperand &A, const SplitOperand &W, float *C, const SplitPtr *Csplit, int ldc, int M, int N, int K, hipStream_t st,
                       const GemmOpts &o, bool tile128) {
    if (o.accumulate || o.ksplit) { set_error("gemm_bf16x3: no accumulate, no split-K (a batch of partial products stands in for it)"); return MDD_ERR_ARG; }
    if (!x3_args_ok(A, W, M, N, K, o.batch)) return MDD_ERR_ARG;
    if (A.period < 0 || W.period < 0) { set_error("gemm_bf16x3: negative operand period %d %d", A.period, W.period); return MDD_ERR_ARG; }
    // large projection: 256x256 tiles, the 8-phase kernel (the single-barrier kernel it is screened against: mdd_diag_gemm_ph8)
    if (!Csplit && o.batch == 1 && M >= 1024 && N >= 512 && !tile128)   // (one product: matrix 0 of either operand whatever its period)
        return launch_gemm_bf16x3_256(X3Form::Phase8, {.p = A.p, .ld = A.ld}, {.p = W.p, .ld = W.ld}, C, ldc, M, N, K, st, o.bias);
    const int tm = (M + XBM - 1) / XBM, tn = (N + XBN - 1) / XBN;   // 128x128 tiles (also batched / split output)
    dim3 grid(tm * tn, 1, o.batch), block(256);
    if (Csplit)
        hipLaunchKernelGGL(gemm_bf16x3_glds_kernel<1>, grid, block, 0, st, A.p.hi, A.p.lo, W.p.hi, W.p.lo, o.bias, (float *)nullptr, Csplit->hi, Csplit->lo,
                           M, N, K, A.ld, W.ld, ldc, A.stride, W.stride, o.sC, tn, A.period, W.period);
    else
        hipLaunchKernelGGL(gemm_bf16x3_glds_kernel<0>, grid, block, 0, st, A.p.hi, A.p.lo, W.p.hi, W.p.lo, o.bias, C, (unsigned short *)nullptr,
                           (unsigned short *)nullptr, M, N, K, A.ld, W.ld, ldc, A.stride, W.stride, o.sC, tn, A.period, W.period);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// C[M,N] (row stride ldc) = opA . opB^T (+ bias[N]) as split-bf16 x3, for the training step (the sibling of gemm_f32x6_ops): both operands
// are written into xs_a / xs_b as bf16 hi/lo planes with the contraction along their rows' contiguous axis (transposed on the way when the
// operand is stored [K, *]).  S > 1: the K axis is cut into S chunks that run as a batch of partial products (the planes' K axis is
// contiguous, so chunk s starts s*Kc elements into every row), summed afterwards.
int gemm_bf16x3_ops(const GemmOperand &A, const GemmOperand &B, const float *bias, float *C, int ldc, int M, int N, int K, int S, DeviceBuf &xs_a,
                    DeviceBuf &xs_b, DeviceBuf &part, hipStream_t st) {
    if (S < 1 || (S > 1 && (bias || ldc != N))) { set_error("gemm_bf16x3_ops: %d chunks need ldc == N and no bias", S); return MDD_ERR_ARG; }
    if (A.period || B.period) { set_error("gemm_bf16x3_ops: one product, no operand period"); return MDD_ERR_ARG; }
    const int Kc = ((K + S - 1) / S + 31) / 32 * 32, Kp = S * Kc;
    if (int rc = xs_a.need((size_t)M * Kp)) return rc;
    if (int rc = xs_b.need((size_t)N * Kp)) return rc;
    SplitPtr sa{reinterpret_cast<unsigned short *>(xs_a.p), reinterpret_cast<unsigned short *>(xs_a.p) + (size_t)M * Kp};
    SplitPtr sb{reinterpret_cast<unsigned short *>(xs_b.p), reinterpret_cast<unsigned short *>(xs_b.p) + (size_t)N * Kp};
    if (int rc = A.k_major ? launch_transpose_split(A.p, A.ld, K, M, Kp, sa.hi, sa.lo, st) : launch_split_rows(A.p, A.ld, (size_t)M, K, Kp, sa.hi, sa.lo, st)) return rc;
    if (int rc = B.k_major ? launch_transpose_split(B.p, B.ld, K, N, Kp, sb.hi, sb.lo, st) : launch_split_rows(B.p, B.ld, (size_t)N, K, Kp, sb.hi, sb.lo, st)) return rc;
    if (S == 1) return launch_gemm_bf16x3({.p = sa, .ld = Kp}, {.p = sb, .ld = Kp}, C, nullptr, ldc, M, N, Kp, st, {.bias = bias});
    return sum_parts(part, S, (size_t)M * N, C, st, [&](float *p) {
        return launch_gemm_bf16x3({.p = sa, .ld = Kp, .stride = Kc}, {.p = sb, .ld = Kp, .stride = Kc}, p, nullptr, N, M, N, Kc, st, {.batch = S, .sC = (long)M * N});
    });
}

}  // namespace mdd
