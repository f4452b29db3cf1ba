// Best reading of an error network: the max-product sweep over the network of ctc_confnet.hip with a backtrace -- decoding constrained to
// the error network of the canonical sequence (an "extended recognition network").  Inputs as mdd_ctc_confnet: each utterance has J slots,
// slot j offers C weighted entries w[j, k], k != blank "slot j emits label k", k == blank "slot j emits nothing".  A reading picks one entry
// r_j per slot.  The call returns
//     max over readings r and over CTC paths pi of r's labels of   sum_j w[j, r_j] + sum_{t < len} logp[t, pi_t]
// with the reading and the frames of every emitted label.  It is the best PAIR of reading and alignment -- NOT the reading with the
// largest summed likelihood over its alignments (that sum is what mdd_ctc_confnet's marginals are made of).
//
// No reference counterpart.  The states and transitions are those of DESIGN.md "Error network" with max for (+):
//   Src_t(j, k) = max_{k' != k} X_t(j, k')                            (k' == blank included: the blank state feeds every label)
//   E_t(0, k) = B_t;   E_t(j+1, k) = max(skip_j + E_t(j, k), Src_t(j, k))
//   X_t(j, k) = lp[t, k] + max(X_{t-1}(j, k), w[j, k] + E_{t-1}(j, k));   X_t(j, blank) = lp[t, blank] + max_k' X_{t-1}(j, k')
//   before frame 0: X = -inf, E_{-1}(j, k) = sum_{m < j} skip_m
//   score = End(J):  End(0) = B_{T-1} (0 without frames),  End(j+1) = max(skip_j + End(j), max_k X_{T-1}(j, k))
// "All but k" is the top-two trick: the largest and second largest of X_t(j, .) with their classes; lane k takes the second where it holds
// the first (top_two: two wave-wide maxima by DPP, wave_max_dpp of ctc_wave.h, and the lowest lane that holds each).  fp64 additions and
// comparisons only, no exp or log.
//
// One workgroup of 16 waves per utterance, a template form per 64 classes, lanes over k, a wave owning ceil(J / 16) consecutive slots: the
// shape of ctc_confnet_kernel, whose block fold carries over because the chain along the slots is linear in max-plus too.  In the first
// phase of a frame a wave steps its slots and walks the chain through its block as if nothing entered it, and publishes the block's end and
// its sum of skips; behind a barrier every wave folds the blocks in front of it into what does enter and completes E_t of its slots.
// Backpointers, one record of 2 NP + 1 64-bit words per (t, j) in the workspace:
//   enter[p]   bit k: X_t(j, k) was entered from E_{t-1}(j, k) (else: stayed in X_{t-1}(j, k))
//   source[p]  bit k: E_t(j+1, k) came from Src_t(j, k) (else: slot j was skipped), decided on the completed E_t(j, k)
//   top        the classes of the largest and second largest X_t(j, .), 16 bits each
// After the last frame one lane walks them back -- at most T + J dependent steps -- and leaves reading and seg in LDS, which the
// workgroup then copies out; path it writes itself.
// Ties (exactly equal values): staying in a label wins over entering it; the source of the nearer slot wins over skipping that slot, also
// at the end (ending in slot j wins over skipping it); among classes the lower one wins.  E_t(j, k) of the fold and the sequential chain
// differ by the rounding of a differently ordered sum of skips: such values are not ties, and either choice scores the same to rounding.
// No atomics: the same bits on every call.
#include <math.h>

#include "ctc_confnet.h"
#include "ctc_host.h"
#include "ctc_wave.h"

namespace mdd {

typedef unsigned long long u64;

struct ConfnetBestArgs {
    const float *logp; int T, B, C;
    const int *len; const float *w; int slot_stride;
    const int *nslots; int Jmax, blank;
    double *score; int *reading, *status, *path, *seg;
    u64 *ws; size_t ws_utt;         // the backpointer records, [T, J, 2 NP + 1] per utterance
};

// The largest (m1, class i1) and second largest (m2, class i2 != i1) of the wave's 64 NP values; lanes at or past C hold -inf and are never
// named.  Equal values: the lower class.
template <int NP> __device__ __forceinline__ void top_two(const double (&v)[NP], int lane, int C, double &m1, int &i1, double &m2, int &i2) {
    double m = v[0];
    for (int p = 1; p < NP; p++) m = fmax(m, v[p]);
    m1 = wave_max_dpp(m);
    i1 = -1;
    for (int p = 0; p < NP; p++) {
        const u64 bal = __ballot(v[p] == m1 && p * 64 + lane < C);
        if (i1 < 0 && bal) i1 = p * 64 + __ffsll(bal) - 1;
    }
    double r = -INFINITY;
    for (int p = 0; p < NP; p++) if (p * 64 + lane != i1) r = fmax(r, v[p]);
    m2 = wave_max_dpp(r);
    i2 = -1;
    for (int p = 0; p < NP; p++) {
        const u64 bal = __ballot(v[p] == m2 && p * 64 + lane != i1 && p * 64 + lane < C);
        if (i2 < 0 && bal) i2 = p * 64 + __ffsll(bal) - 1;
    }
}

template <int NP> __global__ __launch_bounds__(64 * CN_WAVES) void ctc_confnet_best_kernel(ConfnetBestArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    __shared__ int feasible;
    constexpr int R = 2 * NP + 1;
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int T = a.T, B = a.B, C = a.C, blank = a.blank, Jmax = a.Jmax;
    int Tb = a.len[b];
    if (Tb > T) Tb = T;
    if (Tb < 0) Tb = 0;
    int J = a.nslots[b];
    bool bad = J < 0 || J > Jmax;
    if (bad) J = 0;
    const float *w = a.w + (size_t)b * a.slot_stride * C;
    int *reading = a.reading + (size_t)b * a.slot_stride;
    int *seg = a.seg ? a.seg + (size_t)b * a.slot_stride * 2 : nullptr;
    int *path = a.path ? a.path + (size_t)b * T : nullptr;
    int mine = 0;
    for (int i = tid; i < J * C; i += nthr) { const float v = w[i]; mine |= (v != v) || v == INFINITY; }
    bad = __syncthreads_or(mine) || bad;
    if (bad) {
        if (tid == 0) { a.score[b] = NAN; a.status[b] = MDD_ALIGN_BAD_TARGET; }
        for (int j = tid; j < Jmax; j += nthr) {
            reading[j] = -1;
            if (seg) { seg[2 * j] = -1; seg[2 * j + 1] = -1; }
        }
        if (path) for (int t = tid; t < T; t += nthr) path[t] = -1;
        return;
    }

    const int JC = J * C;
    double *X = reinterpret_cast<double *>(sm), *E = X + JC, *S = E + JC;      // S: Src_t(j, k), kept for the source bit
    double *pend = S + JC, *aend = pend + CN_WAVES * C;        // a wave's block as one step of the chain: max(pend[wave, k], aend[wave] + .)
    double *skip = aend + CN_WAVES, *all_j = skip + J, *apre = all_j + J, *end_j = apre + J;
    int *rd_s = reinterpret_cast<int *>(end_j + J + 1), *seg_s = rd_s + J;      // the backtrace's reading [J] and seg [J, 2]
    const int per = (J + CN_WAVES - 1) / CN_WAVES;             // a wave owns `per` consecutive slots
    const int j0 = wave * per < J ? wave * per : J, j1 = j0 + per < J ? j0 + per : J;
    for (int j = tid; j < J; j += nthr) {
        skip[j] = (double)w[(size_t)j * C + blank];
        all_j[j] = -INFINITY;
        rd_s[j] = blank;
        seg_s[2 * j] = seg_s[2 * j + 1] = -1;
    }
    __syncthreads();
    if (tid == 0) {         // end_j holds pre(j) = sum_{m < j} skip_m until the sweep is over
        double s = 0.0;
        for (int j = 0; j < J; j++) { end_j[j] = s; s += skip[j]; }
    }
    __syncthreads();
    for (int i = tid; i < JC; i += nthr) { X[i] = -INFINITY; E[i] = end_j[i / C]; }
    __syncthreads();

    u64 *rec = a.ws + (size_t)b * a.ws_utt;
    const size_t lp_step = (size_t)B * C;
    const float *lp_b = a.logp + (size_t)b * C;
    double blk = 0.0;       // B_t
    for (int t = 0; t < Tb; t++) {
        const float *lp = lp_b + (size_t)t * lp_step;
        u64 *rec_t = rec + (size_t)t * J * R;
        // the slots' own step, and the chain along the wave's block as if nothing entered it: eloc, with apre the skips in front
        double eloc[NP], run = 0.0;
        float lpk[NP], wn[NP];      // wn: the next slot's weights, requested a slot ahead of their use
        for (int p = 0; p < NP; p++) {
            const int k = p * 64 + lane;
            eloc[p] = -INFINITY;
            lpk[p] = k < C ? lp[k] : 0.f;
            wn[p] = (k < C && j0 < j1) ? w[j0 * C + k] : 0.f;
        }
        for (int j = j0; j < j1; j++) {
            double v[NP], m1, m2;
            int i1, i2;
            u64 ent[NP];
            const double all_prev = all_j[j], sk = skip[j];
            for (int p = 0; p < NP; p++) {
                const int k = p * 64 + lane;
                const float wc = wn[p];
                bool enter = false;
                v[p] = -INFINITY;
                if (k < C) {
                    const int i = j * C + k;
                    if (j + 1 < j1) wn[p] = w[i + C];
                    if (k == blank) {
                        v[p] = (double)lpk[p] + all_prev;
                    } else {
                        const double stay = X[i], en = (double)wc + E[i];
                        enter = en > stay;
                        v[p] = (double)lpk[p] + (enter ? en : stay);
                    }
                }
                ent[p] = __ballot(enter);
            }
            top_two<NP>(v, lane, C, m1, i1, m2, i2);
            for (int p = 0; p < NP; p++) {
                const int k = p * 64 + lane;
                const double src = k == i1 ? m2 : m1;
                if (k < C) { X[j * C + k] = v[p]; S[j * C + k] = src; E[j * C + k] = eloc[p]; }
                eloc[p] = fmax(sk + eloc[p], src);
            }
            if (lane == 0) {
                all_j[j] = m1;
                apre[j] = run;
                u64 *r = rec_t + (size_t)j * R;
                for (int p = 0; p < NP; p++) r[p] = ent[p];
                r[2 * NP] = (u64)(unsigned)i1 | ((u64)(unsigned)i2 << 16);
            }
            run += sk;
        }
        for (int p = 0; p < NP; p++) {
            const int k = p * 64 + lane;
            if (k < C) pend[wave * C + k] = eloc[p];
        }
        if (lane == 0) aend[wave] = run;
        blk += (double)lp[blank];
        __syncthreads();
        // what enters the block: B_t through the blocks in front; then E_t of the own slots and where E_t of the next slot comes from
        for (int p = 0; p < NP; p++) {
            const int k = p * 64 + lane;
            double ein = blk;
            if (k < C) for (int v = 0; v < wave; v++) ein = fmax(aend[v] + ein, pend[v * C + k]);
            for (int j = j0; j < j1; j++) {
                bool source = false;
                if (k < C) {
                    const double e = fmax(E[j * C + k], apre[j] + ein);
                    E[j * C + k] = e;
                    source = S[j * C + k] >= skip[j] + e;
                }
                const u64 bal = __ballot(source);
                if (lane == 0) rec_t[(size_t)j * R + NP + p] = bal;
            }
        }
        __syncthreads();
    }

    if (tid == 0) {
        double e = blk;
        for (int j = 0; j < J; j++) { end_j[j] = e; e = fmax(skip[j] + e, all_j[j]); }
        const bool ok = e != -INFINITY;
        a.score[b] = e;
        a.status[b] = ok ? MDD_ALIGN_OK : MDD_ALIGN_INFEASIBLE;
        feasible = ok;
        if (ok) {
            // the end: the last slot that emits, found from behind; slots behind it emit nothing
            int j = J, t = Tb - 1, k = blank, seg_end = -1;
            bool in_state = false;
            while (j > 0 && !in_state) {
                --j;
                if (all_j[j] >= skip[j] + end_j[j]) { in_state = true; k = (int)(rec[((size_t)t * J + j) * R + 2 * NP] & 0xffff); }
            }
            while (in_state) {      // at X_t(j, k), a finite state: t >= 0
                if (k == blank) {
                    if (path) path[t] = -1;
                    if (t == 0) { --t; break; }     // (no finite blank state at frame 0)
                    k = (int)(rec[((size_t)(t - 1) * J + j) * R + 2 * NP] & 0xffff);
                    --t;
                    continue;
                }
                if (path) path[t] = j;
                if (seg_end < 0) { seg_end = t + 1; rd_s[j] = k; }
                const bool enter = (rec[((size_t)t * J + j) * R + (k >> 6)] >> (k & 63)) & 1;
                --t;
                if (!enter && t >= 0) continue;
                seg_s[2 * j] = t + 1;
                seg_s[2 * j + 1] = seg_end;
                seg_end = -1;
                in_state = false;
                if (t < 0) break;       // E_{-1}(j, k): the slots in front are skipped
                while (j > 0) {         // at E_t(j, k): the link from slot j - 1
                    --j;
                    const u64 *r = rec + ((size_t)t * J + j) * R;
                    if ((r[NP + (k >> 6)] >> (k & 63)) & 1) {
                        const int i1 = (int)(r[2 * NP] & 0xffff), i2 = (int)((r[2 * NP] >> 16) & 0xffff);
                        k = i1 != k ? i1 : i2;
                        in_state = true;
                        break;
                    }
                }
            }
            if (path) for (; t >= 0; --t) path[t] = -1;     // B_t: nothing emitted yet
        }
    }
    __syncthreads();
    const bool ok = feasible != 0;
    for (int j = tid; j < Jmax; j += nthr) {
        const bool in = ok && j < J;
        reading[j] = in ? rd_s[j] : -1;
        if (seg) { seg[2 * j] = in ? seg_s[2 * j] : -1; seg[2 * j + 1] = in ? seg_s[2 * j + 1] : -1; }
    }
    if (path) for (int t = (ok ? Tb : 0) + tid; t < T; t += nthr) path[t] = -1;
}

static int init_confnet_best_attributes() {
    const void *k[] = {(const void *)ctc_confnet_best_kernel<1>, (const void *)ctc_confnet_best_kernel<2>, (const void *)ctc_confnet_best_kernel<3>,
                       (const void *)ctc_confnet_best_kernel<4>};
    for (const void *f : k) MDD_HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CN_LDS_LIMIT));
    return MDD_OK;
}

}  // namespace mdd

extern "C" int64_t mdd_ctc_confnet_best_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t Jmax) {
    if (T <= 0 || B <= 0 || C <= 0 || Jmax < 0) return 0;
    return (int64_t)8 * T * B * Jmax * (2 * ((C + 63) / 64) + 1);
}

extern "C" int mdd_ctc_confnet_best(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, const float *w_dev,
                                    int32_t slot_stride, const int32_t *nslots_dev, int32_t Jmax, int32_t blank, double *score_dev,
                                    int32_t *reading_dev, int32_t *status_dev, int32_t *path_dev, int32_t *seg_dev, void *workspace_dev,
                                    int64_t workspace_bytes, void *stream) {
    using namespace mdd;
    const char *what = !logp_dev ? "logp_dev is NULL" : !len_dev ? "len_dev is NULL" : !w_dev ? "w_dev is NULL" : !nslots_dev ? "nslots_dev is NULL"
                     : !score_dev ? "score_dev is NULL" : !reading_dev ? "reading_dev is NULL" : !status_dev ? "status_dev is NULL"
                     : T <= 0 ? "T <= 0" : B <= 0 ? "B <= 0" : C <= 0 ? "C <= 0" : C > 256 ? "C > 256"
                     : (blank < 0 || blank >= C) ? "blank outside [0, C)" : Jmax < 0 ? "Jmax < 0" : Jmax > slot_stride ? "Jmax > slot_stride"
                     : Jmax > mdd_ctc_confnet_max_slots(C) ? "Jmax too long for LDS (mdd_ctc_confnet_max_slots)" : nullptr;
    if (what) { set_error("mdd_ctc_confnet_best: %s", what); return MDD_ERR_ARG; }
    const int64_t need = mdd_ctc_confnet_best_workspace_bytes(T, B, C, Jmax);
    if (workspace_dev && workspace_bytes < need)
        return refuse_workspace("mdd_ctc_confnet_best", "mdd_ctc_confnet_best_workspace_bytes", workspace_bytes, need);
    static OncePerDevice once;
    if (int rc = once_per_device(once, init_confnet_best_attributes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    StreamWorkspace ws;
    if (int rc = ws.acquire(workspace_dev, need, st)) return rc;
    const int NP = (C + 63) / 64;
    ConfnetBestArgs a;
    a.logp = logp_dev; a.T = T; a.B = B; a.C = C; a.len = len_dev; a.w = w_dev; a.slot_stride = slot_stride; a.nslots = nslots_dev;
    a.Jmax = Jmax; a.blank = blank; a.score = score_dev; a.reading = reading_dev; a.status = status_dev; a.path = path_dev; a.seg = seg_dev;
    a.ws = ws.as<u64>(); a.ws_utt = (size_t)T * Jmax * (2 * NP + 1);
    const size_t lds = confnet_lds_doubles(C, Jmax) * 8;
    const dim3 grid(B), block(64 * CN_WAVES);
    switch (NP) {
        case 1: hipLaunchKernelGGL(ctc_confnet_best_kernel<1>, grid, block, lds, st, a); break;
        case 2: hipLaunchKernelGGL(ctc_confnet_best_kernel<2>, grid, block, lds, st, a); break;
        case 3: hipLaunchKernelGGL(ctc_confnet_best_kernel<3>, grid, block, lds, st, a); break;
        default: hipLaunchKernelGGL(ctc_confnet_best_kernel<4>, grid, block, lds, st, a); break;
    }
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { set_error("ctc confnet best kernel launch failed: %s", hipGetErrorString(le)); return MDD_ERR_HIP; }
    return MDD_OK;
}
