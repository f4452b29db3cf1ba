// BiLSTM recurrence: one launch per time step, both directions in the same grid.
//
// Reference: torch.nn.LSTM as used by BatchRNN.forward (AA/models/model_ctc.py:36-49) and by the text
// encoder (:150,198): gate order i,f,g,o, zero initial state, every padded step is processed, the
// reverse direction starts at t = T-1.
//
// Per step and direction:  G^T[n,b] = sum_k Whh[n,k] h_prev[b,k]   (n = 4H gate rows, b = batch)
// is computed with v_mfma_f32_16x16x4_f32 with the GATE rows on the MFMA row axis and the batch on
// the column axis.  Gate rows are stored permuted (n' = unit*4 + gate) so that the four accumulator
// registers of a lane are exactly i,f,g,o of one (unit, batch) pair: the cell update needs no
// cross-lane traffic and no LDS.  A wave owns 4 hidden units x 16 batch rows; a workgroup = 4 waves
// = 4 batch tiles of the same 4 units; grid = (H/4 unit tiles, 2 directions, ceil(B/64)).
// The k axis is split over the four 16-lane groups of the wave in contiguous quarters (the MFMA
// only requires A and B to agree on k), so every lane streams H/4 contiguous floats of one Whh row
// and of one h_prev row.
//
// The launch boundary is the step-to-step dependency (all-to-all over hidden units): per the
// MI355X price list a dependent kernel boundary (~1.5 us) is cheaper than any in-launch grid sync.
// The exact-fp32 training step's part of the family is here too (train.h): the gate-row packing and W_hh transpose of its weight
// layouts and the per-step backward, lstm_bwd_step_kernel.  Every per-step kernel, forward or backward, goes through launch_steps().
#include "lstm_persist.h"
#include "train.h"

namespace mdd {

// ---- generic variant (any H % 4 == 0; row-major Whh', h and c): used for small test geometries
// VEC: 0 scalar k loop (any H % 4 == 0), 1 float4 k loop (H % 16 == 0), N > 1: a lane's quarter of the contraction is exactly N
// float4 steps (24 at H = 384, 16 at H = 256) and all of its loads are issued before the first MFMA (one L2 round trip per step).
template <int VEC>
__global__ __launch_bounds__(256) void lstm_step_kernel(LstmStepArgs a, int s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ut = blockIdx.x, d = blockIdx.y;
    const int b0 = (blockIdx.z * 4 + wave) * 16;
    if (b0 >= a.B) return;  // wave-uniform
    const int H = a.H, B = a.B, KQ = H >> 2;
    const int t = d ? (a.T - 1 - s) : s;
    const int li = lane & 15, kq = lane >> 4;
    const int b = b0 + li, bc = b < B ? b : B - 1;
    const float *hprev = a.hbuf + ((size_t)((s & 1) ^ 1) * 2 + d) * B * H;
    float *hnext = a.hbuf + ((size_t)(s & 1) * 2 + d) * B * H;

    // the epilogue's operands do not depend on the product: request them first, so the step pays one memory round trip, not two
    const int u = ut * 4 + kq;
    const size_t ci = ((size_t)d * B + bc) * H + u;
    const float4 g4 = *reinterpret_cast<const float4 *>(a.gx + (((size_t)t * B + bc) * 2 + d) * 4 * H + u * 4);
    const float cold = s > 0 ? a.cbuf[ci] : 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
        const float *wp = a.whh + ((size_t)d * 4 * H + ut * 16 + li) * H + kq * KQ;  // A[row li][k quarter kq]
        const float *hp = hprev + (size_t)bc * H + kq * KQ;                            // B[k quarter kq][col li]
        if (VEC > 1) {
            float4 w4[VEC > 1 ? VEC : 1], h4[VEC > 1 ? VEC : 1];
#pragma unroll
            for (int n = 0; n < VEC; n++) { w4[n] = *reinterpret_cast<const float4 *>(wp + 4 * n); h4[n] = *reinterpret_cast<const float4 *>(hp + 4 * n); }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n = 0; n < VEC; n++) {    // same accumulation order as the float4 loop below: one chain, x y z w per step
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[n].x, h4[n].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[n].y, h4[n].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[n].z, h4[n].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[n].w, h4[n].w, acc, 0, 0, 0);
            }
        } else if (VEC) {
#pragma unroll 8
            for (int k = 0; k < KQ; k += 4) {
                float4 w4 = *reinterpret_cast<const float4 *>(wp + k);
                float4 h4 = *reinterpret_cast<const float4 *>(hp + k);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.x, h4.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.y, h4.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.z, h4.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.w, h4.w, acc, 0, 0, 0);
            }
        } else {
            for (int k = 0; k < KQ; k++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[k], hp[k], acc, 0, 0, 0);
        }
    }
    // D layout: col = lane&15 (batch), row = 4*(lane>>4) + r  ->  unit = ut*4 + (lane>>4), gate = r
    if (b < B) {
        const float ig = sigmoid_f(acc[0] + g4.x), fg = sigmoid_f(acc[1] + g4.y);
        const float gg = tanhf(acc[2] + g4.z), og = sigmoid_f(acc[3] + g4.w);
        const bool hold = d && a.seqlen && t >= a.seqlen[b];     // reverse direction has not reached this row's last step yet
        const float cn = hold ? 0.f : fg * cold + ig * gg;
        const float hn = hold ? 0.f : og * tanhf(cn);
        a.cbuf[ci] = cn;
        hnext[(size_t)b * H + u] = hn;
        if (a.gates_save) {   // train mode: what the backward sweep needs (lstm_bwd_step_kernel below, lstm_bwd.hip)
            const size_t si = (((size_t)t * B + b) * 2 + d) * H + u;
            *reinterpret_cast<float4 *>(a.gates_save + si * 4) = make_float4(ig, fg, gg, og);
            a.c_save[si] = cn;
        }
        const size_t oi = ((size_t)t * B + b) * 2 * H + d * H + u;
        if (a.out_raw) a.out_raw[oi] = hn;
        const float ov = a.oscale ? hn * a.oscale[d * H + u] + a.oshift[d * H + u] : hn;
        if (a.out && a.out != a.out_raw) a.out[oi] = ov;
        if (a.out_split.hi) {
            __bf16 hb = (__bf16)ov, lb = (__bf16)(ov - (float)hb);
            a.out_split.hi[oi] = *reinterpret_cast<unsigned short *>(&hb);
            a.out_split.lo[oi] = *reinterpret_cast<unsigned short *>(&lb);
        }
    }
}

// ---- packed variant (H % 16 == 0): every global access of the k-loop is a fully coalesced 1 KB read.
// Whh is repacked at weight-load time into the exact order the lanes consume it,
//   Wp[d][ut][j][lane][m] = Whh'[d][ut*16 + (lane&15)][16 j + 4 (lane>>4) + m]
// and h is exchanged between steps in the same consumer order,
//   hp[parity][d][bt][j][lane][m] = h[bt*16 + (lane&15)][16 j + 4 (lane>>4) + m]
// (a producer wave owns k = 4 ut .. 4 ut+3 for 16 batch rows: 64 contiguous floats), and c lives in
// producer order cp[d][bt][ut][lane].  Two independent accumulators (even / odd float4 components) keep
// the MFMA pipe at its 32-cycle issue rate instead of the 40-cycle dependent latency; lstm_layer_f32_kernel (lstm_f32.hip)
// repeats this accumulation order and the cell update bit for bit.
template <int J>
__global__ __launch_bounds__(256, 1) void lstm_step_packed_kernel(LstmStepArgs a, int s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ut = blockIdx.x, d = blockIdx.y;
    const int NBT = (a.B + 15) >> 4, NUT = a.H >> 2;
    const int bt = blockIdx.z * 4 + wave;
    if (bt >= NBT) return;  // wave-uniform
    const int H = a.H, B = a.B;
    const int t = d ? (a.T - 1 - s) : s;
    const int li = lane & 15, uu = lane >> 4;
    const int b = bt * 16 + li, u = ut * 4 + uu;
    const size_t hplane = (size_t)2 * NBT * J * 256;  // floats per parity
    const float4 *hp = reinterpret_cast<const float4 *>(a.hbuf + ((s & 1) ^ 1) * hplane) + ((size_t)(d * NBT + bt) * J) * 64 + lane;
    const float4 *wp = reinterpret_cast<const float4 *>(a.whh) + ((size_t)(d * NUT + ut) * J) * 64 + lane;
    const size_t ci = ((size_t)(d * NBT + bt) * NUT + ut) * 64 + lane;

    float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float cold = 0.f;
    if (b < B) {
        g4 = *reinterpret_cast<const float4 *>(a.gx + (((size_t)t * B + b) * 2 + d) * 4 * H + u * 4);
        if (s > 0) cold = a.cbuf[ci];
    }
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    if (s > 0) {
        float4 w4[J], h4[J];
#pragma unroll
        for (int j = 0; j < J; j++) { w4[j] = wp[j * 64]; h4[j] = hp[j * 64]; }
        // keep every load ahead of the first MFMA: the whole k-panel (2 x J KB per wave) is in flight at once,
        // so the step pays ONE L2 round trip instead of one per k-slice (hipcc otherwise sinks the loads)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < J; j++) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[j].x, h4[j].x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[j].y, h4[j].y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[j].z, h4[j].z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[j].w, h4[j].w, acc1, 0, 0, 0);
        }
    }
    if (b < B) {
        const float gi = (acc0[0] + acc1[0]) + g4.x;
        const float gf = (acc0[1] + acc1[1]) + g4.y;
        const float gg = (acc0[2] + acc1[2]) + g4.z;
        const float go = (acc0[3] + acc1[3]) + g4.w;
        const float ig = gate_sigmoid(gi), fg = gate_sigmoid(gf), cg = gate_tanh(gg), og = gate_sigmoid(go);
        const bool hold = d && a.seqlen && t >= a.seqlen[b];
        const float cn = hold ? 0.f : fg * cold + ig * cg;
        const float hn = hold ? 0.f : og * gate_tanh(cn);
        a.cbuf[ci] = cn;
        float *hnext = a.hbuf + (s & 1) * hplane;
        hnext[(((size_t)(d * NBT + bt) * J + (ut >> 2)) * 64 + (ut & 3) * 16 + li) * 4 + uu] = hn;
        const size_t oi = ((size_t)t * B + b) * 2 * H + d * H + u;
        if (a.out_raw) a.out_raw[oi] = hn;
        const float ov = a.oscale ? hn * a.oscale[d * H + u] + a.oshift[d * H + u] : hn;
        if (a.out && a.out != a.out_raw) a.out[oi] = ov;
        if (a.out_split.hi) {
            __bf16 hb = (__bf16)ov, lb = (__bf16)(ov - (float)hb);
            a.out_split.hi[oi] = *reinterpret_cast<unsigned short *>(&hb);
            a.out_split.lo[oi] = *reinterpret_cast<unsigned short *>(&lb);
        }
    }
}

// ---- split-bf16 tiled variant: the recurrent product on the bf16 matrix cores, operands shared through LDS.
// Per step and direction  G^T[4H x B] = Whh'[4H x H] . h^T[H x B]  is a small GEMM that every step re-reads in
// full, so the step is bound by L2->CU traffic, not by arithmetic.  A workgroup owns RT*16 gate rows (RT*4 hidden
// units) x 64 batch rows and stages its Whh' panel and its h panel ONCE in LDS (bf16 hi/lo planes: the same 4
// bytes per element as fp32), instead of every wave streaming both operands from L2 (2.6x less L2 traffic than the
// packed fp32 variant at B=256).  Products are the bf16x3 form Ah.Bh + Ah.Bl + Al.Bh on v_mfma_f32_16x16x32_bf16
// (3/16 of the fp32 MFMA time).  The D layout (col = batch, 4 accumulator registers = i,f,g,o of one unit) and the
// cell epilogue are those of the fp32 variants.  h is exchanged between steps as row-major [dir][B][H] hi/lo planes
// (the producer lane writes its bf16 pair), c stays fp32 row-major.
// LDS: Wh | Wl : RT*16 rows, hh | hl : 64 rows, each row H*2 bytes + 16 pad (conflict-free ds_read_b128 fragments).
template <int RT, int H>
__global__ __launch_bounds__(256, 1) void lstm_step_x3_kernel(LstmStepArgs a, int s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int ROWB = H * 2 + 16, WROWS = RT * 16, CPR = H / 8;   // CPR: 16-byte chunks per row
    unsigned char *Wh = smem, *Wl = Wh + WROWS * ROWB, *Hh = Wl + WROWS * ROWB, *Hl = Hh + 64 * ROWB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = blockIdx.y, B = a.B;
    const int r0 = blockIdx.x * WROWS;            // first gate row (permuted order) of this workgroup
    const int b0 = blockIdx.z * 64;               // first batch row
    const int t = d ? (a.T - 1 - s) : s;
    const int li = lane & 15, uu = lane >> 4;
    const int b = b0 + wave * 16 + li;
    const size_t hplane = (size_t)2 * B * H;      // elements per (parity, hi|lo) plane: [dir][B][H]
    const unsigned short *hprev_h = a.hsplit + (size_t)(((s & 1) ^ 1) * 2 + 0) * hplane + (size_t)d * B * H;
    const unsigned short *hprev_l = a.hsplit + (size_t)(((s & 1) ^ 1) * 2 + 1) * hplane + (size_t)d * B * H;

    f32x4 acc[RT];
#pragma unroll
    for (int i = 0; i < RT; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (s > 0) {
        // ---- stage both panels: all loads in flight at once, then one LDS write pass
        constexpr int WCH = WROWS * CPR, HCH = 64 * CPR;              // chunks per plane
        static_assert(WCH % 256 == 0 && HCH % 256 == 0, "panel sizes must be whole passes of the workgroup");
        constexpr int NW = WCH / 256, NH = HCH / 256;
        u32x4 wvh[NW], wvl[NW], hvh[NH], hvl[NH];
        const unsigned short *wsrc_h = a.whh_split.hi + ((size_t)d * 4 * H + r0) * H;
        const unsigned short *wsrc_l = a.whh_split.lo + ((size_t)d * 4 * H + r0) * H;
        // branch-free: rows past B are clamped to the last valid row (their output columns are never stored)
#pragma unroll
        for (int i = 0; i < NW; i++) {
            const int q = tid + 256 * i;                              // rows are contiguous: chunk q = row q/CPR
            wvh[i] = *reinterpret_cast<const u32x4 *>(wsrc_h + (size_t)q * 8);
            wvl[i] = *reinterpret_cast<const u32x4 *>(wsrc_l + (size_t)q * 8);
        }
#pragma unroll
        for (int i = 0; i < NH; i++) {
            const int q = tid + 256 * i, row = q / CPR, c = q - row * CPR;
            const int br = min(b0 + row, B - 1);
            hvh[i] = *reinterpret_cast<const u32x4 *>(hprev_h + (size_t)br * H + c * 8);
            hvl[i] = *reinterpret_cast<const u32x4 *>(hprev_l + (size_t)br * H + c * 8);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NW; i++) {
            const int q = tid + 256 * i, row = q / CPR, c = q - row * CPR;
            *reinterpret_cast<u32x4 *>(Wh + row * ROWB + c * 16) = wvh[i];
            *reinterpret_cast<u32x4 *>(Wl + row * ROWB + c * 16) = wvl[i];
        }
#pragma unroll
        for (int i = 0; i < NH; i++) {
            const int q = tid + 256 * i, row = q / CPR, c = q - row * CPR;
            *reinterpret_cast<u32x4 *>(Hh + row * ROWB + c * 16) = hvh[i];
            *reinterpret_cast<u32x4 *>(Hl + row * ROWB + c * 16) = hvl[i];
        }
        __syncthreads();
        // ---- this wave: batch tile `wave` (16 columns) x RT row tiles
        const unsigned char *hb_h = Hh + (wave * 16 + li) * ROWB + uu * 16;
        const unsigned char *hb_l = Hl + (wave * 16 + li) * ROWB + uu * 16;
#pragma unroll 4
        for (int ks = 0; ks < H / 32; ks++) {
            const bf16x8 bh = *reinterpret_cast<const bf16x8 *>(hb_h + ks * 64);
            const bf16x8 bl = *reinterpret_cast<const bf16x8 *>(hb_l + ks * 64);
#pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(Wh + (rt * 16 + li) * ROWB + uu * 16 + ks * 64);
                const bf16x8 al = *reinterpret_cast<const bf16x8 *>(Wl + (rt * 16 + li) * ROWB + uu * 16 + ks * 64);
                acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc[rt], 0, 0, 0);
                acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc[rt], 0, 0, 0);
                acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc[rt], 0, 0, 0);
            }
        }
    }
    if (b >= B) return;
    unsigned short *hnext_h = a.hsplit + (size_t)((s & 1) * 2 + 0) * hplane + (size_t)d * B * H;
    unsigned short *hnext_l = a.hsplit + (size_t)((s & 1) * 2 + 1) * hplane + (size_t)d * B * H;
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        const int u = (r0 >> 2) + rt * 4 + uu;    // D: col = lane&15 (batch), row = 4*(lane>>4) + r -> unit uu of the tile, gate r
        const float4 g4 = *reinterpret_cast<const float4 *>(a.gx + (((size_t)t * B + b) * 2 + d) * 4 * H + u * 4);
        const size_t ci = ((size_t)d * B + b) * H + u;
        const float cold = s > 0 ? a.cbuf[ci] : 0.f;
        const float ig = fast_sigmoid(acc[rt][0] + g4.x), fg = fast_sigmoid(acc[rt][1] + g4.y);
        const float cg = fast_tanh(acc[rt][2] + g4.z), og = fast_sigmoid(acc[rt][3] + g4.w);
        const bool hold = d && a.seqlen && t >= a.seqlen[b];
        const float cn = hold ? 0.f : fg * cold + ig * cg;
        const float hn = hold ? 0.f : og * fast_tanh(cn);
        a.cbuf[ci] = cn;
        {
            const unsigned int pk = split_h(hn);
            hnext_h[(size_t)b * H + u] = (unsigned short)(pk & 0xffffu);
            hnext_l[(size_t)b * H + u] = (unsigned short)(pk >> 16);
        }
        const size_t oi = ((size_t)t * B + b) * 2 * H + d * H + u;
        if (a.out_raw) a.out_raw[oi] = hn;
        const float ov = a.oscale ? hn * a.oscale[d * H + u] + a.oshift[d * H + u] : hn;
        if (a.out && a.out != a.out_raw) a.out[oi] = ov;
        if (a.out_split.hi) {
            __bf16 hb = (__bf16)ov, lb = (__bf16)(ov - (float)hb);
            a.out_split.hi[oi] = *reinterpret_cast<unsigned short *>(&hb);
            a.out_split.lo[oi] = *reinterpret_cast<unsigned short *>(&lb);
        }
    }
}

// ------------------------------------------------------------------------------------------------ LSTM weight layouts
// reference W [4H, K] per direction (gate-major rows g*H + u)  <->  packed W' [2][4H][K] with rows u*4 + g
__global__ void pack_gates_kernel(const float *__restrict__ w_fwd, const float *__restrict__ w_rev, float *__restrict__ packed, int H, int K, int to_packed,
                                  float *__restrict__ out_fwd, float *__restrict__ out_rev) {
    const size_t n = (size_t)2 * 4 * H * K;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % K);
        const size_t row = i / K;                      // d*4H + u*4 + g
        const int d = (int)(row / (4 * H)), rr = (int)(row % (4 * H)), u = rr >> 2, g = rr & 3;
        const size_t j = ((size_t)g * H + u) * K + k;  // index inside the direction's reference tensor
        if (to_packed) packed[i] = (d ? w_rev : w_fwd)[j];
        else (d ? out_rev : out_fwd)[j] = packed[i];
    }
}
int launch_pack_gates(const float *w_fwd, const float *w_rev, float *packed, int H, int K, hipStream_t st) {
    hipLaunchKernelGGL(pack_gates_kernel, dim3(2048), dim3(256), 0, st, w_fwd, w_rev, packed, H, K, 1, (float *)nullptr, (float *)nullptr);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}
int launch_unpack_gates(const float *packed, float *out_fwd, float *out_rev, int H, int K, hipStream_t st) {
    hipLaunchKernelGGL(pack_gates_kernel, dim3(2048), dim3(256), 0, st, (const float *)nullptr, (const float *)nullptr, const_cast<float *>(packed), H, K, 0, out_fwd, out_rev);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}
// Whh' [2][4H][H] -> WhhT [2][H][4H]  (the backward step reads Whh' down its columns)
__global__ void transpose_whh_kernel(const float *__restrict__ w, float *__restrict__ wt, int H) {
    const size_t n = (size_t)2 * 4 * H * H;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % H);
        const size_t row = i / H;
        const int d = (int)(row / (4 * H)), nrow = (int)(row % (4 * H));
        wt[((size_t)d * H + k) * 4 * H + nrow] = w[i];
    }
}
int launch_transpose_whh(const float *w, float *wt, int H, hipStream_t st) {
    hipLaunchKernelGGL(transpose_whh_kernel, dim3(2048), dim3(256), 0, st, w, wt, H);
    MDD_LAUNCH_CHECK(); return MDD_OK;
}

// ------------------------------------------------------------------------------------------------ LSTM backward (BPTT), one launch per step
// Backward order s = 0..T-1 visits time t_s = T-1-s (forward direction) / s (reverse direction).  Launch s, for its 16 hidden
// units k and 16 batch rows b:
//   dh[b,k]   = dout[t_s, b, d, k] + sum_n DG[t_prev][b, d, n] * Whh'[d][n][k]         (t_prev = the time visited by launch s-1)
//   then the cell backward of (t_s, b, k): with the saved gates i,f,g,o, c_t and c_{t-1},
//     do = dh * tanh(c_t) * o(1-o);   dc = dh * o * (1 - tanh(c_t)^2) + dc_carry
//     di = dc * g * i(1-i);  df = dc * c_{t-1} * f(1-f);  dg = dc * i * (1-g^2);  dc_carry = dc * f
//   DG[t_s][b, d, k*4 + {i,f,g,o}] = pre-activation gradients (what the weight-gradient GEMMs and the next launch read).
// The contraction over n = 4H is split over the four waves of the workgroup (one quarter each, v_mfma_f32_16x16x4_f32 with the
// units on the MFMA row axis) and combined through LDS; the launch boundary is the step-to-step dependency.
// NQ4 > 0: H is a compile-time multiple of 16 and a lane's share of the contraction is NQ4 float4 steps (24 at H = 384, 16 at
// H = 256): ALL of its loads are issued before the first MFMA, so a step pays one L2 round trip instead of one per unrolled group.
template <int NQ4>
__global__ __launch_bounds__(256, 1) void lstm_bwd_step_kernel(LstmBwdArgs a, int s) {
    __shared__ float red[4][16 * 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kt = blockIdx.x, d = blockIdx.y, b0 = blockIdx.z * 16;
    const int H = a.H, B = a.B, T = a.T, G = 4 * H;
    const int t = d ? s : (T - 1 - s);
    const int tprev = d ? s - 1 : (T - s);                 // time visited by the previous launch
    const int li = lane & 15, kq = lane >> 4;
    // the cell backward's operands (saved gates, cell states, the carried cell gradient, the upstream gradient) do not depend on the
    // product: every thread requests those of its (unit, batch) element before the contraction, one memory round trip per step
    const int ul = tid >> 4, bl = tid & 15;
    const int u = kt * 16 + ul, b = b0 + bl;
    const bool live = u < H && b < B;
    const int uc = min(u, H - 1), bcl = min(b, B - 1);
    const size_t si = (((size_t)t * B + bcl) * 2 + d) * H + uc;
    const float4 gt = *reinterpret_cast<const float4 *>(a.gates + si * 4);
    const float ct = a.cst[si];
    const int tp = d ? t + 1 : t - 1;                       // the forward pass's previous time of this direction
    const float cprev = (tp >= 0 && tp < T) ? a.cst[(((size_t)tp * B + bcl) * 2 + d) * H + uc] : 0.f;
    const size_t ci = ((size_t)d * B + bcl) * H + uc;
    const float dc_in = s > 0 ? a.dc[ci] : 0.f;
    const float dout_v = a.dout[((size_t)t * B + bcl) * 2 * H + d * H + uc];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) {
        // wave w contracts n in [w*G/4, (w+1)*G/4); inside the wave the four 16-lane groups take contiguous quarters of that range
        const int nq = G / 16, n0 = wave * (G / 4) + kq * nq;
        const int bb = min(b0 + li, B - 1);
        const float *wp = a.whhT + ((size_t)d * H + min(kt * 16 + li, H - 1)) * G + n0;               // A[row = unit li][n]
        const float *gp = a.dg + (((size_t)tprev * B + bb) * 2 + d) * G + n0;                        // B[n][col = batch li]
        if (NQ4 > 0) {
            float4 w4[NQ4 > 0 ? NQ4 : 1], g4[NQ4 > 0 ? NQ4 : 1];
#pragma unroll
            for (int n = 0; n < NQ4; n++) { w4[n] = *reinterpret_cast<const float4 *>(wp + 4 * n); g4[n] = *reinterpret_cast<const float4 *>(gp + 4 * n); }
            __builtin_amdgcn_sched_barrier(0);
            f32x4 a1 = acc, a2 = acc, a3 = acc;           // four chains: the dependent-issue latency of the fp32 MFMA exceeds its issue time
#pragma unroll
            for (int n = 0; n < NQ4; n++) {
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[n].x, g4[n].x, acc, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[n].y, g4[n].y, a1, 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[n].z, g4[n].z, a2, 0, 0, 0);
                a3 = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[n].w, g4[n].w, a3, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) acc[r] = (acc[r] + a1[r]) + (a2[r] + a3[r]);
        } else {
            for (int n = 0; n < nq; n++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[n], gp[n], acc, 0, 0, 0);
        }
    }
    // D layout: col = lane&15 (batch), row = 4*(lane>>4) + r (unit within the tile)
#pragma unroll
    for (int r = 0; r < 4; r++) red[wave][(4 * kq + r) * 16 + li] = acc[r];
    __syncthreads();
    // one thread per (unit, batch) of the tile
    if (!live) return;
    const float dh_rec = (red[0][ul * 16 + bl] + red[1][ul * 16 + bl]) + (red[2][ul * 16 + bl] + red[3][ul * 16 + bl]);
    const float dh = dout_v + dh_rec;
    const float th = tanhf(ct);
    const float d_o = dh * th * gt.w * (1.f - gt.w);
    const float dcell = dh * gt.w * (1.f - th * th) + dc_in;
    const float d_i = dcell * gt.z * gt.x * (1.f - gt.x);
    const float d_f = dcell * cprev * gt.y * (1.f - gt.y);
    const float d_g = dcell * gt.x * (1.f - gt.z * gt.z);
    a.dc[ci] = dcell * gt.y;
    *reinterpret_cast<float4 *>(a.dg + (((size_t)t * B + b) * 2 + d) * G + u * 4) = make_float4(d_i, d_f, d_g, d_o);
}

// One launch per time step of a per-step kernel (forward: LstmStepArgs, backward: LstmBwdArgs); the caller checks the launches
template <class Args>
static void launch_steps(void (*kernel)(Args, int), dim3 grid, size_t smem, const Args &a, hipStream_t st) {
    for (int s = 0; s < a.T; s++) hipLaunchKernelGGL(kernel, grid, dim3(256), smem, st, a, s);
}
// grid of the forward kernels: (grid_x, 2 directions, 64-row batch blocks)
static dim3 fwd_grid(int grid_x, const LstmStepArgs &a) { return dim3(grid_x, 2, (a.B + 63) / 64); }
template <int RT, int H>
static void launch_x3_steps(const LstmStepArgs &a, hipStream_t st) {
    constexpr int ROWB = H * 2 + 16;
    launch_steps(lstm_step_x3_kernel<RT, H>, fwd_grid(4 * H / (RT * 16), a), (size_t)2 * (RT * 16 + 64) * ROWB, a, st);
}

int init_lstm_attributes() {
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)lstm_step_x3_kernel<2, 384>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)lstm_step_x3_kernel<2, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return MDD_OK;
}

int launch_lstm_layer_train(const LstmStepArgs &a, hipStream_t st) {
    if (a.H % 4 != 0 || a.T <= 0 || a.B <= 0 || a.packed || a.hsplit) { set_error("lstm (train): bad arguments T=%d B=%d H=%d", a.T, a.B, a.H); return MDD_ERR_ARG; }
    launch_steps(a.H == 384 ? lstm_step_kernel<24> : a.H == 256 ? lstm_step_kernel<16> : a.H % 16 == 0 ? lstm_step_kernel<1> : lstm_step_kernel<0>, fwd_grid(a.H / 4, a), 0, a, st);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

int launch_lstm_layer(const LstmStepArgs &a, hipStream_t st) {
    if (a.H % 4 != 0 || a.T <= 0 || a.B <= 0) { set_error("lstm: bad shape T=%d B=%d H=%d", a.T, a.B, a.H); return MDD_ERR_ARG; }
    if (a.hsplit && a.H != 384 && a.H != 256) { set_error("lstm: split-bf16 step built for H in {256,384}"); return MDD_ERR_ARG; }
    if (!a.hsplit && a.packed && a.H != 384 && a.H != 256) { set_error("lstm: packed layout built for H in {256,384}"); return MDD_ERR_ARG; }
    if (a.hsplit) a.H == 384 ? launch_x3_steps<2, 384>(a, st) : launch_x3_steps<2, 256>(a, st);
    else launch_steps(!a.packed ? lstm_step_kernel<0> : a.H == 384 ? lstm_step_packed_kernel<24> : lstm_step_packed_kernel<16>, fwd_grid(a.H / 4, a), 0, a, st);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

int launch_lstm_bwd(const LstmBwdArgs &a, hipStream_t st) {
    if (a.H % 4) { set_error("lstm backward: H must be a multiple of 4"); return MDD_ERR_ARG; }
    launch_steps(a.H == 384 ? lstm_bwd_step_kernel<24> : a.H == 256 ? lstm_bwd_step_kernel<16> : lstm_bwd_step_kernel<0>,
                 dim3((a.H + 15) / 16, 2, (a.B + 15) / 16), 0, a, st);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}

}  // namespace mdd
