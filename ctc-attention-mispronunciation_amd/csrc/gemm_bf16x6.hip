// "f32x6": fp32-grade NT GEMM on the bf16 matrix cores.  C[M,N] = A[M,K] . W[N,K]^T (+ bias).
//
// gfx950 has no TF32 and its fp32 MFMA runs at 1/16 of the bf16 rate (it executes on the fp32 vector lanes).  An fp32 value is,
// exactly, the sum of THREE bf16 numbers -- hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid): 3 x 8 significand bits = the
// 24 of fp32 -- so a product of two fp32 values is the sum of nine bf16 x bf16 products, each exact in fp32.  The six largest
// (hi.hi; hi.mid, mid.hi; hi.lo, lo.hi, mid.mid) carry everything down to 2^-24 of the product, i.e. to fp32's own rounding; the
// three dropped ones (mid.lo, lo.mid, lo.lo) are below it.  Six bf16 MFMAs cost 6/16 of the fp32 MFMA they replace.
// What decides the accuracy is not the dropped terms but the ORDER of accumulation: hi.hi is summed in an accumulator of its own
// (one rounding per 32 products) and the five small products in a second one (their roundings happen at 2^-8 of the scale),
// combined once at the end.  Emulated and measured (tests/test_gpu_parity.py::test_gemm_f32x6_accuracy): closer to the float64
// product than ATen's fp32 GEMM on the CPU and ~3x closer than the exact-fp32 MFMA GEMM, which is one rounding per 2 products.
//
// This file holds the kernel, its launchers and gemm_f32x6_ops, the training step's entry.  The operand planes are made in split.hip (and by
// the producers that write them directly: the fused conv front end, the f32x6 BiLSTM layer); the timing entries are in diag.hip.
#include "train.h"

namespace mdd {

// ---- the kernel: a (64 RT) x 128 tile of C per workgroup, FOUR waves (one per SIMD, 512 registers each), K-tile 32; RT = 3 or 4 (template
// parameter; which launch takes which: x6_choose_tile, gemm_raster.h).
// A wave owns 16 RT rows x all 128 columns: RT x 8 MFMA tiles x THREE accumulator sets -- hh (hi.hi), sm (the five small products), tot (hh
// flushed into it every X6_FLUSH K-tiles: at K = 1952 one chain of 61 roundings was measured at 1.3x ATen's error, segments of 8
// are below it).  RT = 3: 288 accumulator registers, which is what the one-wave-per-SIMD shape is for.  RT = 4 (256 x 128, the large
// projections' tile): hh and sm alone are the 256 registers of the accumulation file, and `tot`, which is idle but for one addition per
// segment, lives in the 112 KB of LDS the stages leave (28 of a lane's 32 chunks, X6_TOT below; 4 in registers): the per-K-tile cost that
// does not grow with the rows -- the W pieces and fragment reads, the wait and the barrier -- is spread over a third more MFMAs, and per
// MFMA a quarter fewer W bytes come through LDS and from beyond L2.  The arithmetic of a C element is the same in both: tot = 0, then
// tot = tot + hh per segment, then (tot + sm) + bias.  What it gave (1 - 2.5 % of kernel time: the flush now costs LDS bandwidth of all
// four waves at once) is in profiles/gemm_rt4_notes.txt.  RT = 3 is the training step's split-K instantiation and every small launch.
// Operand paths (what the first forms of this kernel taught, profiles/round3_gemm_f32x6_notes.txt):
//  * A: a wave's rows are nobody else's, so its A fragments never touch LDS: 3 RT (nine, twelve) 16-byte-per-lane global loads per K-tile straight into
//    registers, issued a whole K-tile ahead.  The planes are K-tile-major (launch_split3), so one load instruction is 1 KB of
//    contiguous memory in fragment order.
//  * W: shared by the four waves, streamed HBM/L2 -> LDS by LDS-DMA (24 KB per K-tile, six pieces per wave, XOR-swizzled on the
//    source side so that fragment reads are conflict-free), two stages; fragments are read two column tiles at a time, one pair ahead of
//    the MFMAs that use them -- never in a burst: four waves reading a K-tile's worth of fragments at once behind a barrier took
//    ~780 cycles (LDS bandwidth), a third of the K-tile's MFMA time.
//  * every memory instruction goes out alone between MFMA groups (a burst stalls the issuing wave, and with one wave per SIMD nobody
//    else feeds the matrix pipe meanwhile); one vmcnt(0) + barrier per K-tile, a whole K-tile after the requests.
// The two MFMA-fed accumulator sets live in the accumulation file ("+a" asm MFMAs: the compiler otherwise shuttles a set between the
// files on every K-tile) and the flush sits between two loops, not in a conditional inside one (same reason).  The W fragment is the
// MFMA's first operand, so a lane's four accumulator registers are four consecutive columns of one C row: 16-byte stores.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void6;
constexpr int X6_BN = 128, X6_BK = 32, X6_ROW = 64;                   // X6_ROW: bytes per LDS row (32 bf16); a tile's rows: x6_bm(RT) (gemm_raster.h)
constexpr int X6_PW = X6_BN * X6_ROW;                                 // bytes per W plane of a stage (8 KB)
constexpr int X6_STAGE = 3 * X6_PW;                                   // 24 KB
constexpr int X6_NS = 2;                                              // stages
constexpr int X6_NPW = 3 * (X6_BN / 16) / 4;                          // LDS-DMA pieces per wave and K-tile (6)
constexpr int X6_FLUSH = 8;
// RT = 4: where a lane's `tot` lives.  Chunk c = i * 8 + j (row tile i, column tile j; one f32x4) of thread t is at X6_TOT + (c * 256 + t) * 16 bytes
// behind the two W stages -- chunk-major, so a wave's 16-byte reads and writes are 1 KB of consecutive LDS (conflict-free) and a lane only
// ever meets its own data: no barrier, only the wave's own lgkmcnt.  As many chunks as the CU's 160 KB hold beside the stages (28 of the
// 32); the rest stay in registers.  Never an LDS-DMA target.
constexpr int X6_TOT = X6_NS * X6_STAGE, X6_LDS_CU = 160 * 1024;
constexpr int x6_tot_lds(int rt) { return rt < 4 ? 0 : (X6_LDS_CU - X6_TOT) / (256 * 16) < rt * 8 ? (X6_LDS_CU - X6_TOT) / (256 * 16) : rt * 8; }
constexpr int x6_lds_bytes(int rt) { return X6_TOT + x6_tot_lds(rt) * 256 * 16; }

__device__ __forceinline__ bf16x8 x6_frag(const unsigned char *plane, int row, int kbyte) {
    return *reinterpret_cast<const bf16x8 *>(plane + row * X6_ROW + ((((kbyte >> 4) ^ ((row >> 2) & 3))) << 4));
}

// SPLITK (the weight gradients of the training step: few output tiles, a long contraction): the contraction is cut into chunks of K
// elements each and the workgroups walk chunks x tiles VIRTUAL tiles.  In K-tile-major planes chunk s is a contiguous slab of every plane,
// (s * K / 32) * rows * 32 elements in, so a virtual tile is an ordinary tile on shifted plane pointers; it writes its M x N partial
// product (ldc == N) behind the s - 1 before it, and a reduction pass sums them (no atomics: the sum has one fixed order).  tiles_c: output
// tiles per chunk, which arrives in the `ldc` argument (the row stride of a partial product is N); walk.ntiles counts the virtual tiles, which
// are always taken in the row walk (the launcher builds it as chunks x tiles_c and sets walk.tiles_n to the output's column tiles); K is the
// chunk's length.  The instantiation with SPLITK false is the decode path's kernel: every SPLITK expression below folds to the plain
// argument (Ap, Wp, C, ldc), and tile_of to one call of x6_tile_of per round looked at.
template <int RT, bool STAMP, bool SPLITK = false>
__global__ __launch_bounds__(256, 1) void gemm_f32x6_kernel(const unsigned short *__restrict__ Ap, const unsigned short *__restrict__ Wp, size_t a_plane, size_t w_plane,
                                                            const float *__restrict__ bias, float *__restrict__ C, int M, int N, int K, int ldc, X6Walk walk,
                                                            long long *stamps) {
    // STAMP (diagnostic instantiation): per wave, cycles of the K loop in the MFMA stream / waiting for memory / at the barrier
    // -> stamps[(workgroup * 4 + wave) * 4 + {0, 1, 2}]; per workgroup, the shader clock's and the 100 MHz constant clock's ticks around
    // the tile loop -> stamps[X6_STAMP_PHASE_WORDS + workgroup * 2 + {0, 1}]: their quotient is the clock the chip held (tools/gemm_time.py)
    constexpr int X6_RT = RT, X6_BM = x6_bm(RT);
    constexpr int NL = x6_tot_lds(RT);   // chunks of `tot` in LDS (RT = 3: none, `tot` is registers and every NL branch below folds away)
    long long sacc[4] = {0, 0, 0, 0}, stt = 0, clk0 = 0, rt0 = 0;
#define X6_T(i_) do { if (STAMP) { const long long n_ = (long long)__builtin_readcyclecounter(); sacc[i_] += n_ - stt; stt = n_; } } while (0)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem6[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    f32x4 *const totl = reinterpret_cast<f32x4 *>(smem6 + X6_TOT) + tid;   // chunk c of this lane: totl[c * 256]
    // PERSISTENT: a workgroup takes one tile per round of `walk` (one workgroup per CU: no dispatch between tiles, and the next tile's first
    // operands are requested before this tile's epilogue).  Which tile, gemm_raster.h says: by default the 32 workgroups of an XCD
    // (blockIdx.x % 8) share a block of 4 row panels x 8 column tiles per round, so that what the XCD streams through its L2 in the round
    // is 4 A panels and a third of W (in the row walk, MDD_GEMM_X6_RASTER=rows: two or three A panels and the whole of W, twice the bytes).
    // A workgroup with no tile in a round sits it out.  tile_of runs once per tile, on scalars.
    const unsigned short *Ab_ = Ap, *Wb_ = Wp;   // SPLITK: this tile's chunk of the planes and its partial product
    float *Cb_ = C;
#define X6_AB (SPLITK ? Ab_ : Ap)
#define X6_WB (SPLITK ? Wb_ : Wp)
#define X6_LDC (SPLITK ? N : ldc)
    const int tiles_n = walk.tiles_n;
    if (SPLITK) walk.tiles_n = ldc;   // the virtual tiles, always in the row walk: "row" = chunk s, "column" = the chunk's tile
    // the first round from r_ on in which this workgroup has a tile (walk.rounds: none), and that tile
    auto tile_of = [&](int r_, int &m0_, int &n0_) {
        int tm = 0, tn = 0;
        while (r_ < walk.rounds && !x6_tile_of(walk, (int)blockIdx.x, r_, tm, tn)) r_++;
        if (r_ >= walk.rounds) return r_;
        if (SPLITK) {
            const int s = tm, swz = tn;
            Ab_ = Ap + (size_t)s * (K / X6_BK) * M * 32; Wb_ = Wp + (size_t)s * (K / X6_BK) * N * 32; Cb_ = C + (size_t)s * M * N;
            tm = swz / tiles_n; tn = swz % tiles_n;
        }
        m0_ = tm * X6_BM + wave * (16 * X6_RT); n0_ = tn * X6_BN;  // this wave's first row; the workgroup's first column
        return r_;
    };
    int m0 = 0, n0 = 0;
    int rnd = tile_of(0, m0, n0);
    if (rnd >= walk.rounds) return;   // (the whole workgroup: nothing below has been reached)
    f32x4 hh[X6_RT][8], sm[X6_RT][8], tot[X6_RT][8];
    const int l16 = lane & 15, kq = lane >> 4;
    // A fragments straight from the K-tile-major planes: lane (row l16 of row tile i, k-slice kq) reads 16 bytes at ((kt * M + row) * 32 + kq * 8)
    // elements; rows past M are clamped (their C rows are never stored)
    unsigned aoff[X6_RT];
    auto load_a = [&](bf16x8 (&fa)[X6_RT][3], int kt) {
#pragma unroll
        for (int p = 0; p < 3; p++) {
            const unsigned char *base = reinterpret_cast<const unsigned char *>(X6_AB + (size_t)p * a_plane + (size_t)kt * M * 32);
#pragma unroll
            for (int i = 0; i < X6_RT; i++) fa[i][p] = *reinterpret_cast<const bf16x8 *>(base + aoff[i]);
        }
    };
    // W: LDS-DMA pieces of this wave = row groups 2w, 2w+1 (16 rows each) of the three planes
    const unsigned lds0 = (unsigned)(unsigned long long)(lds_void6 *)smem6;
    unsigned voffW[2];
    auto set_tile = [&]() {   // the per-lane offsets of the tile at (m0, n0)
#pragma unroll
        for (int i = 0; i < X6_RT; i++) aoff[i] = (unsigned)(((size_t)min(m0 + i * 16 + l16, M - 1) * 32 + kq * 8) * 2);
#pragma unroll
        for (int g = 0; g < 2; g++) {
            const int row = (wave * 2 + g) * 16 + (lane >> 2), c = (lane & 3) ^ ((row >> 2) & 3);
            voffW[g] = (unsigned)(((size_t)min(n0 + row, N - 1) * 32 + c * 8) * 2);
        }
    };
    set_tile();
    auto piece = [&](int idx, int kt_, unsigned stage_off) {   // idx 0..5: plane idx / 2, row group idx % 2
        const int p = idx >> 1, g = idx & 1;
        const unsigned short *base = X6_WB + (size_t)p * w_plane + (size_t)kt_ * N * 32;
        const unsigned la = lds0 + stage_off + (unsigned)(p * X6_PW + (wave * 2 + g) * 1024);
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voffW[g]), "s"(base), "s"(la) : "memory", "m0");
    };
    const int nk = K / X6_BK;
    const int kq16 = kq * 16;
    bf16x8 faA[X6_RT][3], faB[X6_RT][3];
#pragma unroll
    for (int idx = 0; idx < X6_NPW; idx++) piece(idx, 0, 0u);
    load_a(faA, 0);
#define X6_MFMA(acc_, w_, a_) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc_) : "v"(w_), "v"(a_))
    // One K-tile: fac holds its A fragments, fan receives the next K-tile's.  Column tiles in pairs (jp): the pair's six W fragments are read
    // from LDS one pair ahead; per pair RT rows x 2 columns x 6 products = 36 (48) MFMAs, product-major (six different accumulators in a row),
    // smallest products first, hi.hi last and into its own accumulator.
    auto ktile = [&](int kt, bf16x8 (&fac)[X6_RT][3], bf16x8 (&fan)[X6_RT][3]) {
        const unsigned char *st = smem6 + (kt % X6_NS) * X6_STAGE;
        const unsigned nst = (unsigned)(((kt + 1) % X6_NS) * X6_STAGE);
        // (the last K-tile requests itself again instead of nothing: a branch in front of each of the 15 memory instructions cost more than
        // one K-tile's worth of redundant, never-read loads per 61)
        const int ktn = min(kt + 1, nk - 1);
        bf16x8 fw[2][3][2];
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int jj = 0; jj < 2; jj++) fw[0][p][jj] = x6_frag(st + p * X6_PW, jj * 16 + l16, kq16);
#pragma unroll
        for (int jp = 0; jp < 4; jp++) {
            if (jp + 1 < 4) {
#pragma unroll
                for (int p = 0; p < 3; p++)
#pragma unroll
                    for (int jj = 0; jj < 2; jj++) fw[(jp + 1) & 1][p][jj] = x6_frag(st + p * X6_PW, ((jp + 1) * 2 + jj) * 16 + l16, kq16);
            }
            // memory instructions of the next K-tile, one per product group: the 3 * RT A fragment loads (9: pairs 0, 1; 12: pairs 0, 1), then the
            // 6 W pieces (pairs 1, 2; at RT = 4 pairs 2, 3)
#define X6_MEM(g_) do { const int s_ = jp * 6 + (g_); \
                if (s_ < 3 * X6_RT) { const int p_ = s_ / X6_RT, i_ = s_ % X6_RT; \
                    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(fan[i_][p_]) : "v"(aoff[i_]), "s"(X6_AB + (size_t)p_ * a_plane + (size_t)ktn * M * 32) : "memory"); } \
                else if (s_ < 3 * X6_RT + X6_NPW) piece(s_ - 3 * X6_RT, ktn, nst); } while (0)
#define X6_GROUP(acc_, wp_, ap_) _Pragma("unroll") for (int i = 0; i < X6_RT; i++) { _Pragma("unroll") for (int jj = 0; jj < 2; jj++) X6_MFMA(acc_[i][jp * 2 + jj], fw[jp & 1][wp_][jj], fac[i][ap_]); }
            X6_MEM(0); X6_GROUP(sm, 1, 1)      // mid . mid
            X6_MEM(1); X6_GROUP(sm, 2, 0)      // W lo . A hi
            X6_MEM(2); X6_GROUP(sm, 0, 2)      // W hi . A lo
            X6_MEM(3); X6_GROUP(sm, 1, 0)      // W mid . A hi
            X6_MEM(4); X6_GROUP(sm, 0, 1)      // W hi . A mid
            X6_MEM(5); X6_GROUP(hh, 0, 0)      // hi . hi
#undef X6_GROUP
#undef X6_MEM
        }
        X6_T(0);
        // The next K-tile's A fragments and this wave's W pieces (requested a K-tile ago) are here.  The A loads are asm as well: as C++
        // loads the compiler's wait-count pass, which cannot see the asm LDS-DMA pieces, guarded the next K-tile's first MFMAs with
        // vmcnt(1) / vmcnt(0) that also waited for the loads issued a few instructions earlier (a memory round trip per K-tile).
        // Nothing reads or moves the destination registers before this wait (checked in the ISA: the registers the loads write are the
        // ones the next K-tile's MFMAs read).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        X6_T(1);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // ... everybody's pieces; and every wave is done reading this stage
        X6_T(2);
    };
    if (STAMP) { clk0 = (long long)__builtin_amdgcn_s_memtime(); rt0 = (long long)__builtin_amdgcn_s_memrealtime(); }
    for (;;) {   // ---- one tile per iteration
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0F70);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int i = 0; i < X6_RT; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            hh[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; sm[i][j] = hh[i][j];
            if (i * 8 + j < NL) totl[(i * 8 + j) * 256] = hh[i][j]; else tot[i][j] = hh[i][j];
        }
    if (STAMP) stt = (long long)__builtin_readcyclecounter();
    // Segments of X6_FLUSH K-tiles with the flush of hh into tot BETWEEN them; K-tiles in pairs, so that the two A fragment sets swap roles
    // without a register copy.
    static_assert(X6_FLUSH % 2 == 0 && X6_NS == 2, "K-tiles are taken in pairs");
    for (int kt0 = 0; kt0 < nk; kt0 += X6_FLUSH) {
        const int kt1 = min(kt0 + X6_FLUSH, nk);
        for (int kt = kt0; kt < kt1; kt += 2) {
            ktile(kt, faA, faB);
            if (kt + 1 < kt1) ktile(kt + 1, faB, faA);
        }
        asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");                     // the asm MFMAs' results are read by vector instructions next: their wait states by hand
#pragma unroll
        for (int i = 0; i < X6_RT; i++)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (i * 8 + j < NL) { f32x4 t = totl[(i * 8 + j) * 256]; t += hh[i][j]; totl[(i * 8 + j) * 256] = t; }
                else tot[i][j] += hh[i][j];
                hh[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
    }
    // the next tile's first W stage and A fragments are requested before this tile's epilogue (stage 0 and faA are free: every wave has passed
    // the last K-tile's barrier)
    const int m0c = m0, n0c = n0;
    float *const Cc = SPLITK ? Cb_ : C;
    rnd = tile_of(rnd + 1, m0, n0);
    const bool more = rnd < walk.rounds;
    if (more) {
        set_tile();
#pragma unroll
        for (int idx = 0; idx < X6_NPW; idx++) piece(idx, 0, 0u);
        load_a(faA, 0);
    }
    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
    const int q4 = kq * 4;   // D row = 4 * (lane >> 4) + r = C column, D col = lane & 15 = C row
#pragma unroll
    for (int i = 0; i < X6_RT; i++) {
        const int row = m0c + i * 16 + l16;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int col = n0c + j * 16 + q4;
            if (row >= M || col >= N) continue;
            f32x4 v = (i * 8 + j < NL ? totl[(i * 8 + j) * 256] : tot[i][j]) + sm[i][j];
            if (bias) { v[0] += bias[col]; if (col + 1 < N) v[1] += bias[col + 1]; if (col + 2 < N) v[2] += bias[col + 2]; if (col + 3 < N) v[3] += bias[col + 3]; }
            float *dst = Cc + (size_t)row * X6_LDC + col;
            if (col + 3 < N) *reinterpret_cast<f32x4 *>(dst) = v;
            else for (int r = 0; r < 4 && col + r < N; r++) dst[r] = v[r];
        }
    }
    if (!more) break;
    }   // ---- tiles
#undef X6_MFMA
    if (STAMP && stamps && lane == 0 && blockIdx.x < X6_STAMP_WGS)
        for (int i = 0; i < 4; i++) stamps[((size_t)blockIdx.x * 4 + wave) * 4 + i] = sacc[i];
    if (STAMP && stamps && tid == 0 && blockIdx.x < X6_STAMP_WGS) {
        stamps[X6_STAMP_PHASE_WORDS + (size_t)blockIdx.x * 2] = (long long)__builtin_amdgcn_s_memtime() - clk0;
        stamps[X6_STAMP_PHASE_WORDS + (size_t)blockIdx.x * 2 + 1] = (long long)__builtin_amdgcn_s_memrealtime() - rt0;
    }
#undef X6_T
#undef X6_AB
#undef X6_WB
#undef X6_LDC
}

int init_gemm_x6_attributes() {
    static_assert(x6_lds_bytes(3) == X6_NS * X6_STAGE && x6_lds_bytes(4) <= X6_LDS_CU && x6_tot_lds(4) >= 1, "the RT = 4 tile's tot region fits the CU's LDS");
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)gemm_f32x6_kernel<3, false>, hipFuncAttributeMaxDynamicSharedMemorySize, x6_lds_bytes(3)));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)gemm_f32x6_kernel<3, true>, hipFuncAttributeMaxDynamicSharedMemorySize, x6_lds_bytes(3)));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)gemm_f32x6_kernel<3, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, x6_lds_bytes(3)));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)gemm_f32x6_kernel<4, false>, hipFuncAttributeMaxDynamicSharedMemorySize, x6_lds_bytes(4)));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)gemm_f32x6_kernel<4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, x6_lds_bytes(4)));
    return MDD_OK;
}

template <int RT> static void x6_launch(const X6Walk &walk, hipStream_t st, const unsigned short *A3, const unsigned short *W3, size_t a_plane, size_t w_plane,
                                        const float *bias, float *C, int M, int N, int K, int ldc, long long *stamps) {
    const dim3 grid(walk.grid);   // one persistent workgroup per CU
    if (stamps) hipLaunchKernelGGL((gemm_f32x6_kernel<RT, true>), grid, dim3(256), x6_lds_bytes(RT), st, A3, W3, a_plane, w_plane, bias, C, M, N, K, ldc, walk, stamps);
    else hipLaunchKernelGGL((gemm_f32x6_kernel<RT, false>), grid, dim3(256), x6_lds_bytes(RT), st, A3, W3, a_plane, w_plane, bias, C, M, N, K, ldc, walk, (long long *)nullptr);
}

// A3, W3: three consecutive K-tile-major bf16 planes (hi | mid | lo; launch_split3) of a_plane = M x K / w_plane = N x K elements each
int launch_gemm_f32x6(const unsigned short *A3, size_t a_plane, const unsigned short *W3, size_t w_plane, const float *bias, float *C, int M, int N, int K,
                      int ldc, hipStream_t st, X6Raster raster, long long *stamps, int rt) {
    if (M <= 0 || N <= 0 || K <= 0 || K % X6_BK || ldc % 4 || a_plane != (size_t)M * K || w_plane != (size_t)N * K || (rt != kX6RtRule && rt != 3 && rt != 4)) {
        set_error("gemm_f32x6: bad shape M=%d N=%d K=%d ldc=%d (row tiles %d)", M, N, K, ldc, rt);
        return MDD_ERR_ARG;
    }
    // the tile (x6_choose_tile: RT = 4 where its rounds are no more MFMA time than RT = 3's, or what `rt` forces) and its walk (the block
    // walk, or the row walk where x6_choose_walk falls back)
    const X6Tile tile = x6_choose_tile(M, (N + X6_BN - 1) / X6_BN, raster, rt);
    if (tile.rt == 4) x6_launch<4>(tile.walk, st, A3, W3, a_plane, w_plane, bias, C, M, N, K, ldc, stamps);
    else x6_launch<3>(tile.walk, st, A3, W3, a_plane, w_plane, bias, C, M, N, K, ldc, stamps);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// Split-K form: part[s][M][N] = A[:, s*Kc .. (s+1)*Kc) . W[:, same]^T for s < S, one launch over S x tiles virtual tiles.  A3 / W3: three
// K-tile-major planes each, a_plane / w_plane elements apart, of M (N) rows x S*Kc contraction elements.
int launch_gemm_f32x6_splitk(const unsigned short *A3, size_t a_plane, const unsigned short *W3, size_t w_plane, float *part, int M, int N, int Kc, int S,
                             hipStream_t st) {
    if (!A3 || !W3 || !part || M <= 0 || N <= 0 || Kc <= 0 || Kc % X6_BK || S < 1 || N % 4 || (uintptr_t)part % 16 || (uintptr_t)A3 % 16 || (uintptr_t)W3 % 16 ||
        a_plane % 8 || w_plane % 8 || a_plane < (size_t)M * Kc * S || w_plane < (size_t)N * Kc * S) {
        set_error("gemm_f32x6_splitk: bad shape M=%d N=%d Kc=%d S=%d", M, N, Kc, S);
        return MDD_ERR_ARG;
    }
    const int tn = (N + X6_BN - 1) / X6_BN, tiles_c = x6_ceil_div(M, x6_bm(3)) * tn;   // the split-K instantiation stays on the 192-row tile
    if ((long long)tiles_c * S > (1 << 24)) { set_error("gemm_f32x6_splitk: %d x %d tiles", S, tiles_c); return MDD_ERR_ARG; }
    X6Walk walk = x6_choose_walk(S, tiles_c, kX6Rows);   // S x tiles_c virtual tiles, always in the row walk: their order is the step's own
    walk.tiles_n = tn;
    hipLaunchKernelGGL((gemm_f32x6_kernel<3, false, true>), dim3(walk.grid), dim3(256), x6_lds_bytes(3), st, A3, W3, a_plane, w_plane, (const float *)nullptr, part, M, N, Kc,
                       /* ldc carries */ tiles_c, walk, (long long *)nullptr);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

// C[M,N] (row stride ldc) = opA . opB^T (+ bias[N]) as f32x6, for the training step: opA[m,k] = ta ? A[k*lda + m] : A[m*lda + k], opB[n,k]
// likewise.  Both operands are written as three K-tile-major planes into xs_a / xs_b (transposed on the way when stored [K, *]) with the
// contraction zero-padded to S chunks of whole K-tiles.  S == 1: one launch of the decode path's kernel.  S > 1 (no bias): the split-K
// launch (always in the row walk and on the 192-row tile; `raster` and `rt` are the one-launch form's) into `part` and launch_reduce_parts (into C itself when ldc == N, as the step calls it; else into one more slot of `part`, copied
// out row by row).  The caller has checked x6_ops_ok.
bool x6_ops_ok(const GemmOperand &A, const GemmOperand &B, const float *C, int ldc) {
    return A.ld % 4 == 0 && B.ld % 4 == 0 && ldc % 4 == 0 && (uintptr_t)A.p % 16 == 0 && (uintptr_t)B.p % 16 == 0 && (uintptr_t)C % 16 == 0;
}
int gemm_f32x6_ops(const GemmOperand &A, const GemmOperand &B, const float *bias, float *C, int ldc, int M, int N, int K, int S, DeviceBuf &xs_a,
                   DeviceBuf &xs_b, DeviceBuf &part, hipStream_t st, X6Raster raster, int rt) {
    if (A.period || B.period) { set_error("gemm_f32x6_ops: one product, no operand period"); return MDD_ERR_ARG; }
    if (M <= 0 || N <= 0 || K <= 0 || S < 1 || ldc < N || !x6_ops_ok(A, B, C, ldc) || (S > 1 && bias)) {
        set_error("gemm_f32x6_ops: M=%d N=%d K=%d S=%d lda=%d ldb=%d ldc=%d", M, N, K, S, A.ld, B.ld, ldc); return MDD_ERR_ARG;
    }
    const int nkt = (K + X6_BK - 1) / X6_BK;
    if (S > nkt) S = nkt;
    const int Kc = (nkt + S - 1) / S * X6_BK, Kp = S * Kc;
    const size_t pa = (size_t)M * Kp, pw = (size_t)N * Kp;   // elements per plane (multiples of 32)
    if (int rc = xs_a.need((3 * pa + 1) / 2)) return rc;
    if (int rc = xs_b.need((3 * pw + 1) / 2)) return rc;
    unsigned short *a3 = reinterpret_cast<unsigned short *>(xs_a.p), *w3 = reinterpret_cast<unsigned short *>(xs_b.p);
    if (int rc = A.k_major ? launch_transpose_split3(A.p, K, M, A.ld, Kp, a3, pa, st) : launch_split3_pad(A.p, M, K, A.ld, Kp, a3, pa, st)) return rc;
    if (int rc = B.k_major ? launch_transpose_split3(B.p, K, N, B.ld, Kp, w3, pw, st) : launch_split3_pad(B.p, N, K, B.ld, Kp, w3, pw, st)) return rc;
    if (S == 1) return launch_gemm_f32x6(a3, pa, w3, pw, bias, C, M, N, Kp, ldc, st, raster, nullptr, rt);
    const size_t mn = (size_t)M * N;
    auto partials = [&](float *p) { return launch_gemm_f32x6_splitk(a3, pa, w3, pw, p, M, N, Kc, S, st); };
    if (ldc == N) return sum_parts(part, S, mn, C, st, partials);
    if (int rc = part.need((S + 1) * mn)) return rc;          // one more slot for the sum, copied out row by row
    if (int rc = sum_parts(part, S, mn, part.p + S * mn, st, partials)) return rc;
    return launch_copy_cols(part.p + S * mn, N, 0, C, ldc, 0, (size_t)M, N, false, st);
}

}  // namespace mdd
