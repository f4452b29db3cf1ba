// Minimum-Bayes-risk decode of an N-best list (mdd_nbest_mbr; no reference counterpart: ctcBeamSearch.decode sorts its final list and
// keeps [0]): every pairwise edit distance inside an utterance's list, the expected distance of each hypothesis under the list's own
// weights, and the hypothesis that minimises it.  DESIGN.md "Minimum Bayes risk"; the byte counts are plan.h's mbr_plan, the recurrence
// is mbr.h's mbr_distance.
//
// Three launches on the caller's stream, nothing else:
//   mbr_pack_kernel   one workgroup per utterance: flags it (status, lengths, ids, weights), and packs the ids it has range-checked one
//                     byte each into the workspace (plan.h); a flagged utterance gets its outputs here and is skipped by the other two
//   mbr_dist_kernel   (utterance, block of 16 patterns): a wave takes one pattern n at a time -- its match table peq in LDS, built with one
//                     LDS integer OR per pattern position -- and its 64 lanes take 64 texts m each, so the lanes diverge in text length
//                     alone.  The lane that owns (n, m) stores dist[b, n, m] and adds weight[m] * d to its own partial of risk[n]: chunks
//                     of 64 texts in ascending order, then a butterfly over the lanes.  No floating-point atomics: a fixed order, the same
//                     bits on every call.  With a reference its ids are pattern N: its row gives ref_dist and ref_risk as any row gives
//                     dist and risk (the distance is symmetric).
//   mbr_best_kernel   one workgroup per utterance: the lowest n with weight > 0 and the least risk.
// No id is an index before mbr_pack_kernel has checked it: the other kernels read the packed bytes of unflagged utterances only.
#include "ctc_host.h"
#include "ctc_wave.h"
#include "mbr.h"

namespace mdd {
namespace {

struct MbrArgs {
    const int32_t *ids; int pitch; const int32_t *nids, *status; const double *weight;
    int N, B, C, max_len;
    const int32_t *ref, *ref_len; int ref_pitch;
    int32_t *best; double *risk; int32_t *dist, *ref_dist; double *ref_risk; int32_t *flag;
    uint32_t *packed; int Lp, NP;     // the workspace: [B][Lp / 4][NP]
};

constexpr int kMbrThreads = 64 * kMbrWaves;

__global__ __launch_bounds__(kMbrThreads) void mbr_pack_kernel(MbrArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N, B = a.B;
    __shared__ int s_bad, s_pos;
    if (tid == 0) { s_bad = 0; s_pos = 0; }
    __syncthreads();
    const bool skip = a.status && a.status[b] != 0;
    const int rows = N + (a.ref ? 1 : 0), Jq = a.Lp / 4, NP = a.NP;
    uint32_t *out = a.packed + (size_t)b * Jq * NP;
    if (!skip) {
        bool bad = false, pos = false;
        for (int n = tid; n < N; n += kMbrThreads) pos = pos || a.weight[(size_t)n * B + b] > 0.0;
        // Jq (16, 32, 64, ..) consecutive lanes take one row and read its length once each; they pack the row's words, so they read
        // consecutive ids: a wave holds 64 / Jq rows at a time, or one row in several steps.  The columns behind the rows, up to NP, are
        // zeroed: every word of the utterance's slice is written.
        const int lanes = Jq < 64 ? Jq : 64, per = kMbrThreads / lanes;      // lanes of a row, rows of the workgroup per step
        for (int r = tid / lanes; r < NP; r += per) {
            int len = 0, cap = 0;
            const int32_t *src = nullptr;
            if (r < N) { len = a.nids[(size_t)r * B + b]; cap = a.max_len; src = a.ids + ((size_t)r * B + b) * a.pitch; }
            else if (r < rows) { len = a.ref_len[b]; cap = a.max_len < a.ref_pitch ? a.max_len : a.ref_pitch; src = a.ref + (size_t)b * a.ref_pitch; }
            if (len < 0 || len > cap) { bad = true; len = 0; }
            for (int jq = tid % lanes; jq < Jq; jq += lanes) {
                uint32_t w = 0;
                for (int i = 0; i < 4; i++) {
                    const int j = 4 * jq + i;
                    if (j < len) {                               // ids past a row's length are not read at all
                        const int id = src[j];
                        if ((unsigned)id >= (unsigned)a.C) bad = true; else w |= (uint32_t)id << (8 * i);
                    }
                }
                out[(size_t)jq * NP + r] = w;
            }
        }
        if (bad) s_bad = 1;
        if (pos) s_pos = 1;
    }
    __syncthreads();
    const int flag = skip ? 1 : s_bad ? 2 : s_pos ? 0 : 1;
    if (tid == 0) a.flag[b] = flag;
    if (!flag) return;
    const double nan = __builtin_nan("");
    if (tid == 0) { a.best[b] = -1; if (a.ref_risk) a.ref_risk[b] = nan; }
    for (int n = tid; n < N; n += kMbrThreads) {
        a.risk[(size_t)n * B + b] = nan;
        if (a.ref_dist) a.ref_dist[(size_t)n * B + b] = -1;
    }
    if (a.dist) for (int i = tid; i < N * N; i += kMbrThreads) a.dist[(size_t)b * N * N + i] = -1;
}

__device__ __forceinline__ double wave_sum_f64(double v) {      // __shfl_xor over distances 32, 16, .., 1: every lane the same bits
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int NW>
__global__ __launch_bounds__(kMbrThreads) void mbr_dist_kernel(MbrArgs a) {
    extern __shared__ __align__(16) unsigned char mbr_smem[];
    typedef unsigned long long u64;
    const int b = blockIdx.x;
    if (a.flag[b] != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = a.N, B = a.B, C = a.C, NP = a.NP;
    const int rows = N + (a.ref ? 1 : 0);
    const uint32_t *packed = a.packed + (size_t)b * (a.Lp / 4) * NP;
    u64 *peq = reinterpret_cast<u64 *>(mbr_smem) + (size_t)wave * C * NW;
    const uint32_t *text = packed;
    if (NW == 1) {      // the one-word form: the utterance's packed list in LDS, as far as max_len reaches
        uint32_t *s_text = reinterpret_cast<uint32_t *>(mbr_smem + sizeof(u64) * (size_t)kMbrWaves * C);
        const int used = ((a.max_len + 3) / 4) * NP;
        for (int i = tid; i < used; i += kMbrThreads) s_text[i] = packed[i];
        __syncthreads();
        text = s_text;
    }
    const int row0 = blockIdx.y * kMbrRowsPerBlock;
    const int row1 = row0 + kMbrRowsPerBlock < rows ? row0 + kMbrRowsPerBlock : rows;
    for (int r = row0 + wave; r < row1; r += kMbrWaves) {           // no workgroup barrier from here on: the waves run on their own
        const int plen = r < N ? a.nids[(size_t)r * B + b] : a.ref_len[b];
        for (int i = lane; i < C * NW; i += 64) peq[i] = 0;
        wave_lds_order();
#pragma unroll
        for (int k = 0; k < NW; k++) {
            const int j = 64 * k + lane;
            if (j < plen) {
                const uint32_t c = (text[(size_t)(j >> 2) * NP + r] >> (8 * (j & 3))) & 255u;
                atomicOr(&peq[c * NW + k], 1ull << lane);          // an LDS integer OR: lanes with the same id meet in one word
            }
        }
        wave_lds_order();
        double acc = 0.0;
        for (int m0 = 0; m0 < N; m0 += 64) {
            const int m = m0 + lane;
            if (m < N) {
                const int tlen = a.nids[(size_t)m * B + b];
                const int d = plen == 0 ? tlen : mbr_distance<NW>(peq, text + m, NP, plen, tlen);
                if (r < N) { if (a.dist) a.dist[((size_t)b * N + r) * N + m] = d; }
                else if (a.ref_dist) a.ref_dist[(size_t)m * B + b] = d;
                acc += a.weight[(size_t)m * B + b] * (double)d;
            }
        }
        acc = wave_sum_f64(acc);
        if (lane == 0) { if (r < N) a.risk[(size_t)r * B + b] = acc; else if (a.ref_risk) a.ref_risk[b] = acc; }
        wave_lds_order();                                             // the next pattern's zero fill stays behind this one's reads
    }
}

__global__ __launch_bounds__(kMbrMaxN) void mbr_best_kernel(MbrArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (a.flag[b] != 0) return;
    __shared__ double s_v[kMbrMaxN];
    __shared__ int s_i[kMbrMaxN];
    double v = __builtin_inf();
    int i = a.N;                                                      // "none": past every rank
    if (tid < a.N && a.weight[(size_t)tid * a.B + b] > 0.0) { v = a.risk[(size_t)tid * a.B + b]; i = tid; }
    s_v[tid] = v; s_i[tid] = i;
    __syncthreads();
    for (int h = kMbrMaxN / 2; h; h >>= 1) {
        if (tid < h) {
            const double v2 = s_v[tid + h];
            const int i2 = s_i[tid + h];
            if (i2 < a.N && (s_i[tid] >= a.N || v2 < s_v[tid] || (v2 == s_v[tid] && i2 < s_i[tid]))) { s_v[tid] = v2; s_i[tid] = i2; }
        }
        __syncthreads();
    }
    if (tid == 0) a.best[b] = s_i[0] < a.N ? s_i[0] : -1;
}

template <int NW> int mbr_set_lds() {
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)mbr_dist_kernel<NW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMbrLdsMax));
    return MDD_OK;
}
int init_mbr_attributes() {
    if (int rc = mbr_set_lds<1>()) return rc;
    if (int rc = mbr_set_lds<2>()) return rc;
    if (int rc = mbr_set_lds<4>()) return rc;
    if (int rc = mbr_set_lds<8>()) return rc;
    return mbr_set_lds<16>();
}

template <int NW> void launch_mbr_dist(const MbrArgs &a, const MbrPlan &p, int row_blocks, hipStream_t st) {
    hipLaunchKernelGGL(mbr_dist_kernel<NW>, dim3(a.B, row_blocks), dim3(kMbrThreads), p.smem, st, a);
}

}  // namespace
}  // namespace mdd

using namespace mdd;

extern "C" int64_t mdd_nbest_mbr_workspace_bytes(int32_t N, int32_t B, int32_t C, int32_t max_len) {
    if (!mbr_shape_ok(N, B, C, max_len)) return 0;
    return (int64_t)mbr_plan(N, B, C, max_len).bytes;
}

// In the order of ctc_host.h: refuse, attributes, workspace, launch, check.
extern "C" int mdd_nbest_mbr(const int32_t *ids_dev, int32_t pitch, const int32_t *nids_dev, const int32_t *status_dev, const double *weight_dev,
                             int32_t N, int32_t B, int32_t C, int32_t max_len, const int32_t *ref_dev, const int32_t *ref_len_dev,
                             int32_t ref_pitch, int32_t *best_dev, double *risk_dev, int32_t *dist_dev, int32_t *ref_dist_dev,
                             double *ref_risk_dev, int32_t *flag_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    const bool has_ref = ref_dev && ref_len_dev;
    const char *what = !ids_dev ? "ids_dev is NULL" : !nids_dev ? "nids_dev is NULL" : !weight_dev ? "weight_dev is NULL"
                     : !best_dev ? "best_dev is NULL" : !risk_dev ? "risk_dev is NULL" : !flag_dev ? "flag_dev is NULL"
                     : (N < 1 || N > kMbrMaxN) ? "need 1<=N<=256" : B < 1 ? "B < 1" : (C < 2 || C > 256) ? "need 2<=C<=256"
                     : (max_len < 1 || max_len > kMbrMaxLen || max_len > pitch) ? "need 1<=max_len<=min(pitch, 1024)"
                     : (ref_dev && !ref_len_dev) ? "ref_len_dev is NULL where ref_dev is given"
                     : (!ref_dev && ref_len_dev) ? "ref_dev is NULL where ref_len_dev is given"
                     : (has_ref && ref_pitch < 1) ? "ref_pitch < 1"
                     : (!has_ref && ref_dist_dev) ? "ref_dist_dev without ref_dev" : (!has_ref && ref_risk_dev) ? "ref_risk_dev without ref_dev"
                     : nullptr;
    if (what) { set_error("mdd_nbest_mbr: bad argument (%s)", what); return MDD_ERR_ARG; }
    const MbrPlan p = mbr_plan(N, B, C, max_len);
    if (workspace_dev && workspace_bytes < (int64_t)p.bytes)
        return refuse_workspace("mdd_nbest_mbr", "mdd_nbest_mbr_workspace_bytes", workspace_bytes, (int64_t)p.bytes);
    hipStream_t st = (hipStream_t)stream;
    static OncePerDevice once;
    if (int rc = once_per_device(once, init_mbr_attributes)) return rc;
    StreamWorkspace ws;
    if (int rc = ws.acquire(workspace_dev, (int64_t)p.bytes, st)) return rc;
    MbrArgs a{ids_dev, pitch, nids_dev, status_dev, weight_dev, N, B, C, max_len, ref_dev, ref_len_dev, ref_pitch,
              best_dev, risk_dev, dist_dev, ref_dist_dev, ref_risk_dev, flag_dev, ws.as<uint32_t>(), p.Lp, p.NP};
    hipLaunchKernelGGL(mbr_pack_kernel, dim3(B), dim3(kMbrThreads), 0, st, a);
    const int rows = N + (has_ref ? 1 : 0), row_blocks = (rows + kMbrRowsPerBlock - 1) / kMbrRowsPerBlock;
    switch (p.words) {
        case 1: launch_mbr_dist<1>(a, p, row_blocks, st); break;
        case 2: launch_mbr_dist<2>(a, p, row_blocks, st); break;
        case 4: launch_mbr_dist<4>(a, p, row_blocks, st); break;
        case 8: launch_mbr_dist<8>(a, p, row_blocks, st); break;
        default: launch_mbr_dist<16>(a, p, row_blocks, st); break;
    }
    hipLaunchKernelGGL(mbr_best_kernel, dim3(B), dim3(kMbrMaxN), 0, st, a);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { set_error("mdd_nbest_mbr: kernel launch failed: %s", hipGetErrorString(le)); return MDD_ERR_HIP; }
    return MDD_OK;
}
