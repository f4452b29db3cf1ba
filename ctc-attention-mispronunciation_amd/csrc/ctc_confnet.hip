// Joint per-phoneme posteriors: CTC over an error network (a confusion network, "sausage").  Each utterance has J slots; slot j offers
// C weighted entries w[j, k]: k != blank "slot j emits label k", k == blank "slot j emits nothing".  A reading picks one entry per slot;
// its score is the sum of its weights plus the CTC log-likelihood of the labels it emits.  total = log-sum over all readings,
// post[j, k] = log-sum over the readings that pick entry k in slot j.  With one slot open and the rest fixed this is mdd_ctc_variants.
//
// No reference counterpart.  Formulas (DESIGN.md "Error network"), in the log domain, (+) is log-add.  A state is the slot j of the last
// emission and what was emitted last: X_t(j, k) for k != blank is "label k of slot j at frame t", X_t(j, blank) "a blank after slot j's
// label"; B_t = sum_{s <= t} lp[s, blank] is "nothing emitted yet".  skip_j = w[j, blank].
//   forward   Src_t(j, k) = (+)_{k' != k} X_t(j, k')                  (k' == blank included: the blank state feeds every label)
//             E_t(0, k) = B_t;   E_t(j+1, k) = (skip_j + E_t(j, k)) (+) Src_t(j, k)                 the only chain along the slots
//             X_t(j, k) = lp[t, k] + (X_{t-1}(j, k) (+) (w[j, k] + E_{t-1}(j, k)));   X_t(j, blank) = lp[t, blank] + (+)_k' X_{t-1}(j, k')
//             before frame 0: X = -inf, E_{-1}(j, k) = pre(j) = sum_{m < j} skip_m
//             total = End(J):  End(0) = B_{T-1} (0 without frames),  End(j+1) = (skip_j + End(j)) (+) (+)_k X_{T-1}(j, k)
//   backward  Y_{T-1}(j, k) = lp[T-1, k] + tail(j),  tail(j) = sum_{m > j} skip_m
//             F_t(J, k) = -inf;  F_t(j, k) = (w[j, k] + Y_{t+1}(j, k)) (+) (skip_j + F_t(j+1, k))  for k != blank            mirrored chain
//             V(k') = F_t(j+1, k') for k' != blank, V(blank) = Y_{t+1}(j, blank)
//             Y_t(j, k) = lp[t, k] + (Y_{t+1}(j, k) (+) (+)_{k' != k} V(k'));   Y_t(j, blank) = lp[t, blank] + (+)_k' V(k')
//   marginals post[j, k]     = (+)_{t = 0..T-1} w[j, k] + E_{t-1}(j, k) + Y_t(j, k)                                    k != blank
//             post[j, blank] = (+)_{t = -1..T-2} (+)_{k != blank} E_t(j, k) + skip_j + F_t(j+1, k)      the flow that jumps over slot j
//                              (+) End(j) + skip_j + tail(j)                                             ... and what ends in front of it
// No log-domain subtraction: "all but k" is an exclusive sum across the lanes, a reading that does not exist is exactly -inf.
//
// One workgroup of 16 waves per utterance, a template form per 64 classes (NP = 1..4), lanes over k.  X / Y, E / F and the marginal
// accumulators (backward) are three [J, C] fp64 rows in LDS; that is what bounds J (mdd_ctc_confnet_max_slots).  A wave owns a block of
// ceil(J / 16) consecutive slots.  The chain along the slots is linear -- E(j+1) = skip_j (x) E(j) (+) Src(j) -- so a block is one step of
// it: in the first phase of a frame a wave does its slots' own work and walks the chain through its block as if nothing entered it
// (eloc, and the skips in front of each slot), and publishes the block's end and its sum of skips; behind a barrier every wave folds
// the blocks in front of its own (at most 15 steps) into what does enter, and completes its slots: E(j) = eloc(j) (+) (skips + entry).
// The dependent chain of a frame is ceil(J / 16) + 15 log-adds, not J.  The backward sweep mirrors it from the last block down.  With
// post_dev the forward stores E_t of every frame but the last ([T, J, C] fp64 per utterance, the workspace) and the backward sweep reads
// it back; without, only the forward runs.
// An n-ary log-add is ctc_lse.h's form on more terms: a reference point at the maximum, exp of the fp32 differences, the sum in fp32 in a
// fixed order (butterfly), one log.  The exclusive sum is the butterfly's too: at each level a lane adds the sibling group's sum, which
// does not hold it.  The lane that holds the maximum sums the others against the second maximum when that lies far below (excl_all),
// so every sum has a term near 1.  No atomics: the same bits on every call.
#include <math.h>

#include "ctc_confnet.h"
#include "ctc_host.h"
#include "ctc_lse.h"
#include "ctc_wave.h"

namespace mdd {

struct ConfnetArgs {
    const float *logp; int T, B, C;
    const int *len; const float *w; int slot_stride;
    const int *nslots; int Jmax, blank;
    double *total, *post; int *status;
    double *ws; size_t ws_utt;      // E_t of every frame, [T, J, C] per utterance (doubles)
};

__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_maxf(float v) {
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// inc: the sum over the wave (the same bits in every lane); returns the sum over every lane but the own one.  At each level of the
// butterfly a lane takes the sum of the sibling group, which does not hold it: an exclusive sum without a subtraction.
__device__ __forceinline__ float wave_excl_sum(float &inc) {
    float exc = 0.f;
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_xor(inc, o);
        exc += t;
        inc += t;
    }
    return exc;
}

// (+) over the 64 NP values of a wave
template <int NP> __device__ __forceinline__ double lse_all(const double (&u)[NP]) {
    double m = u[0];
    for (int p = 1; p < NP; p++) m = fmax(m, u[p]);
    m = wave_max(m);
    const double mm = (m == -INFINITY) ? 0.0 : m;
    float s = 0.f;
    for (int p = 0; p < NP; p++) s += fexp((float)(u[p] - mm));
    return mm + (double)flog(wave_sum_butterfly(s));
}

// ex[p] = (+) over every value of the wave but the lane's own v[p]; all = (+) over every value.  The reference point m1 is the maximum
// rounded to fp32 (any point near the maximum serves: the differences are taken in fp64).  The first holder of the maximum has no term
// near 1 in its sum: when the second maximum m2 lies more than EXCL_FAR below, it sums the others against m2 instead (a wave-uniform
// branch), so that no term of weight is lost to the fp32 range.
static constexpr float EXCL_FAR = 40.f;
template <int NP> __device__ __forceinline__ void excl_all(const double (&v)[NP], int lane, double (&ex)[NP], double &all) {
    float mf = (float)v[0];
    for (int p = 1; p < NP; p++) mf = fmaxf(mf, (float)v[p]);
    mf = wave_maxf(mf);
    int ap = -1, al = 0;
    for (int p = 0; p < NP; p++) {
        const unsigned long long bal = __ballot((float)v[p] == mf);
        if (ap < 0 && bal) { ap = p; al = __ffsll(bal) - 1; }
    }
    float m2f = -INFINITY;
    for (int p = 0; p < NP; p++) if (!(p == ap && lane == al)) m2f = fmaxf(m2f, (float)v[p]);
    m2f = wave_maxf(m2f);
    const double mm1 = (mf == -INFINITY) ? 0.0 : (double)mf, mm2 = (m2f == -INFINITY) ? 0.0 : (double)m2f;
    float exq[NP], tot[NP], total = 0.f;
    for (int p = 0; p < NP; p++) {
        tot[p] = fexp((float)(v[p] - mm1));
        exq[p] = wave_excl_sum(tot[p]);
        total += tot[p];
    }
    for (int p = 0; p < NP; p++) {
        float others = 0.f;
        for (int p2 = 0; p2 < NP; p2++) if (p2 != p) others += tot[p2];
        ex[p] = mm1 + (double)flog(exq[p] + others);
    }
    all = mm1 + (double)flog(total);
    if (mf - m2f > EXCL_FAR) {      // also m2 == -inf: the holder's sum is then empty
        float r = 0.f;
        for (int p = 0; p < NP; p++) if (!(p == ap && lane == al)) r += fexp((float)(v[p] - mm2));
        const double far = mm2 + (double)flog(wave_sum_butterfly(r));
        for (int p = 0; p < NP; p++) if (p == ap && lane == al) ex[p] = far;
    }
}

template <int NP> __global__ __launch_bounds__(64 * CN_WAVES) void ctc_confnet_kernel(ConfnetArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int B = a.B, C = a.C, blank = a.blank, Jmax = a.Jmax;
    int Tb = a.len[b];
    if (Tb > a.T) Tb = a.T;
    if (Tb < 0) Tb = 0;
    int J = a.nslots[b];
    bool bad = J < 0 || J > Jmax;
    if (bad) J = 0;
    const float *w = a.w + (size_t)b * a.slot_stride * C;
    double *post = a.post ? a.post + (size_t)b * a.slot_stride * C : nullptr;
    int mine = 0;
    for (int i = tid; i < J * C; i += nthr) { const float v = w[i]; mine |= (v != v) || v == INFINITY; }
    bad = __syncthreads_or(mine) || bad;
    if (bad) {
        if (tid == 0) { a.total[b] = NAN; a.status[b] = MDD_ALIGN_BAD_TARGET; }
        if (post) for (int i = tid; i < Jmax * C; i += nthr) post[i] = NAN;
        return;
    }
    if (post) for (int i = J * C + tid; i < Jmax * C; i += nthr) post[i] = -INFINITY;

    const int JC = J * C;
    double *X = reinterpret_cast<double *>(sm), *E = X + JC, *S = E + JC;
    double *pend = S + JC, *aend = pend + CN_WAVES * C;        // a wave's block as one step of the chain: (+) pend[wave, k], + aend[wave]
    double *skip = aend + CN_WAVES, *all_j = skip + J, *apre = all_j + J, *pre = apre + J, *tail = pre + J + 1, *end_j = tail + J + 1;   // tail[j + 1] = tail(j)
    const int per = (J + CN_WAVES - 1) / CN_WAVES;             // a wave owns `per` consecutive slots
    const int j0 = wave * per < J ? wave * per : J, j1 = j0 + per < J ? j0 + per : J;
    for (int j = tid; j < J; j += nthr) { skip[j] = (double)w[(size_t)j * C + blank]; all_j[j] = -INFINITY; }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int j = 0; j < J; j++) { pre[j] = s; s += skip[j]; }
        pre[J] = s;
        s = 0.0;
        for (int j = J - 1; j >= 0; j--) { tail[j + 1] = s; s += skip[j]; }
        tail[0] = s;
    }
    __syncthreads();
    for (int i = tid; i < JC; i += nthr) { X[i] = -INFINITY; E[i] = pre[i / C]; }
    __syncthreads();

    double *wsE = a.ws + (size_t)b * a.ws_utt;
    const size_t lp_step = (size_t)B * C;
    const float *lp_b = a.logp + (size_t)b * C;
    double blk = 0.0;       // B_t
    for (int t = 0; t < Tb; t++) {
        const float *lp = lp_b + (size_t)t * lp_step;
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
            double v[NP], ex[NP], all;
            const double all_prev = all_j[j], sk = skip[j];
            for (int p = 0; p < NP; p++) {
                const int k = p * 64 + lane;
                const float wc = wn[p];
                v[p] = -INFINITY;
                if (k < C) {
                    const int i = j * C + k;
                    if (j + 1 < j1) wn[p] = w[i + C];
                    v[p] = (double)lpk[p] + (k == blank ? all_prev : wlse2(X[i], (double)wc + E[i]));
                }
            }
            excl_all<NP>(v, lane, ex, all);
            for (int p = 0; p < NP; p++) {
                const int k = p * 64 + lane;
                if (k < C) { X[j * C + k] = v[p]; E[j * C + k] = eloc[p]; }
                eloc[p] = wlse2(sk + eloc[p], ex[p]);
            }
            if (lane == 0) { all_j[j] = all; apre[j] = run; }
            run += sk;
        }
        for (int p = 0; p < NP; p++) {
            const int k = p * 64 + lane;
            if (k < C) pend[wave * C + k] = eloc[p];
        }
        if (lane == 0) aend[wave] = run;
        blk += (double)lp[blank];
        __syncthreads();
        // what enters the block: B_t through the blocks in front; then E_t of the own slots
        const bool store = post && t + 1 < Tb;
        for (int p = 0; p < NP; p++) {
            const int k = p * 64 + lane;
            if (k < C) {
                double ein = blk;
                for (int v = 0; v < wave; v++) ein = wlse2(aend[v] + ein, pend[v * C + k]);
                for (int j = j0; j < j1; j++) {
                    const double e = wlse2(E[j * C + k], apre[j] + ein);
                    E[j * C + k] = e;
                    if (store) wsE[(size_t)t * JC + j * C + k] = e;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        double e = blk;
        for (int j = 0; j < J; j++) { end_j[j] = e; e = wlse2(skip[j] + e, all_j[j]); }
        a.total[b] = e;
        a.status[b] = e == -INFINITY ? MDD_ALIGN_INFEASIBLE : MDD_ALIGN_OK;
    }
    if (!post) return;

    // backward: X holds Y, E holds F_t(j+1, .) at slot j, S the marginals
    for (int i = tid; i < JC; i += nthr) {
        S[i] = -INFINITY;
        if (Tb > 0) X[i] = (double)lp_b[(size_t)(Tb - 1) * lp_step + i % C] + tail[i / C + 1];
    }
    __syncthreads();
    const int bp = blank >> 6, bl = blank & 63;
    for (int tt = Tb - 1; tt >= 0; tt--) {      // the transition from frame tt - 1 (or the start) into frame tt
        {   // the mirrored chain along the wave's block as if nothing entered it from behind
            double gloc[NP], run = 0.0;
            float wn[NP];
            for (int p = 0; p < NP; p++) {
                const int k = p * 64 + lane;
                gloc[p] = -INFINITY;
                wn[p] = (k < C && j0 < j1) ? w[(j1 - 1) * C + k] : 0.f;
            }
            for (int j = j1 - 1; j >= j0; j--) {
                const double sk = skip[j];
                for (int p = 0; p < NP; p++) {
                    const int k = p * 64 + lane;
                    const float wc = wn[p];
                    if (k < C) {
                        const int i = j * C + k;
                        if (j > j0) wn[p] = w[i - C];
                        E[i] = gloc[p];
                        gloc[p] = k != blank ? wlse2((double)wc + X[i], sk + gloc[p]) : -INFINITY;
                    }
                }
                if (lane == 0) apre[j] = run;
                run += sk;
            }
            for (int p = 0; p < NP; p++) {
                const int k = p * 64 + lane;
                if (k < C) pend[wave * C + k] = gloc[p];
            }
            if (lane == 0) aend[wave] = run;
        }
        __syncthreads();
        const float *lp = lp_b + (size_t)(tt > 0 ? tt - 1 : 0) * lp_step;
        double fin[NP];
        for (int p = 0; p < NP; p++) {
            const int k = p * 64 + lane;
            fin[p] = -INFINITY;
            if (k < C) for (int v = CN_WAVES - 1; v > wave; v--) fin[p] = wlse2(aend[v] + fin[p], pend[v * C + k]);
        }
        const double *wsT = wsE + (size_t)(tt > 0 ? tt - 1 : 0) * JC;
        float lpk[NP], wn[NP];
        double en[NP];              // wn, en: the next slot's weights and stored E, requested a slot ahead of their use
        for (int p = 0; p < NP; p++) {
            const int k = p * 64 + lane;
            lpk[p] = (k < C && tt > 0) ? lp[k] : 0.f;
            wn[p] = (k < C && j0 < j1) ? w[j0 * C + k] : 0.f;
            en[p] = (k < C && j0 < j1 && tt > 0) ? wsT[j0 * C + k] : 0.0;
        }
        for (int j = j0; j < j1; j++) {
            double u[NP], vv[NP], y[NP];
            const double sk = skip[j], ap = apre[j];
            for (int p = 0; p < NP; p++) {
                const int k = p * 64 + lane;
                const float wc = wn[p];
                const double ec = en[p];
                u[p] = vv[p] = y[p] = -INFINITY;
                if (k < C) {
                    const int i = j * C + k;
                    if (j + 1 < j1) {
                        wn[p] = w[i + C];
                        if (tt > 0) en[p] = wsT[i + C];
                    }
                    const double e = tt > 0 ? ec : pre[j];
                    y[p] = X[i];
                    if (k != blank) {
                        const double fn = wlse2(E[i], ap + fin[p]);
                        S[i] = wlse2(S[i], (double)wc + e + y[p]);
                        u[p] = e + sk + fn;
                        vv[p] = fn;
                    } else {
                        vv[p] = y[p];
                    }
                }
            }
            const double over = lse_all<NP>(u);
            for (int p = 0; p < NP; p++)
                if (p == bp && lane == bl) S[j * C + blank] = wlse2(S[j * C + blank], over);
            if (tt > 0) {
                double ex[NP], all;
                excl_all<NP>(vv, lane, ex, all);
                for (int p = 0; p < NP; p++) {
                    const int k = p * 64 + lane;
                    if (k < C) X[j * C + k] = (double)lpk[p] + (k == blank ? all : wlse2(y[p], ex[p]));
                }
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < JC; i += nthr) {
        const int j = i / C, k = i - j * C;
        double v = S[i];
        if (k == blank) v = wlse2(v, end_j[j] + skip[j] + tail[j + 1]);
        post[i] = v;
    }
}

static int init_confnet_attributes() {
    const void *k[] = {(const void *)ctc_confnet_kernel<1>, (const void *)ctc_confnet_kernel<2>, (const void *)ctc_confnet_kernel<3>,
                       (const void *)ctc_confnet_kernel<4>};
    for (const void *f : k) MDD_HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CN_LDS_LIMIT));
    return MDD_OK;
}

}  // namespace mdd

extern "C" int32_t mdd_ctc_confnet_max_slots(int32_t C) {
    if (C < 2 || C > 256) return -1;
    return (int32_t)((mdd::CN_LDS_LIMIT / 8 - 8 - (size_t)mdd::CN_WAVES * (C + 1)) / ((size_t)3 * C + 6));
}

extern "C" int64_t mdd_ctc_confnet_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t Jmax, int32_t want_post) {
    if (T <= 0 || B <= 0 || C <= 0 || Jmax < 0 || !want_post) return 0;
    return (int64_t)8 * T * B * C * Jmax;
}

extern "C" int mdd_ctc_confnet(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, const float *w_dev,
                               int32_t slot_stride, const int32_t *nslots_dev, int32_t Jmax, int32_t blank, double *total_dev, double *post_dev,
                               int32_t *status_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    using namespace mdd;
    const char *what = !logp_dev ? "logp_dev is NULL" : !len_dev ? "len_dev is NULL" : !w_dev ? "w_dev is NULL" : !nslots_dev ? "nslots_dev is NULL"
                     : !total_dev ? "total_dev is NULL" : !status_dev ? "status_dev is NULL" : T <= 0 ? "T <= 0" : B <= 0 ? "B <= 0"
                     : C <= 0 ? "C <= 0" : C > 256 ? "C > 256" : (blank < 0 || blank >= C) ? "blank outside [0, C)" : Jmax < 0 ? "Jmax < 0"
                     : Jmax > slot_stride ? "Jmax > slot_stride" : Jmax > mdd_ctc_confnet_max_slots(C) ? "Jmax too long for LDS (mdd_ctc_confnet_max_slots)"
                     : nullptr;
    if (what) { set_error("mdd_ctc_confnet: %s", what); return MDD_ERR_ARG; }
    const int64_t need = mdd_ctc_confnet_workspace_bytes(T, B, C, Jmax, post_dev != nullptr);
    if (workspace_dev && workspace_bytes < need) return refuse_workspace("mdd_ctc_confnet", "mdd_ctc_confnet_workspace_bytes", workspace_bytes, need);
    static OncePerDevice once;
    if (int rc = once_per_device(once, init_confnet_attributes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    StreamWorkspace ws;
    if (int rc = ws.acquire(workspace_dev, need, st)) return rc;
    ConfnetArgs a;
    a.logp = logp_dev; a.T = T; a.B = B; a.C = C; a.len = len_dev; a.w = w_dev; a.slot_stride = slot_stride; a.nslots = nslots_dev;
    a.Jmax = Jmax; a.blank = blank; a.total = total_dev; a.post = post_dev; a.status = status_dev; a.ws = ws.as<double>();
    a.ws_utt = (size_t)T * C * Jmax;
    const size_t lds = confnet_lds_doubles(C, Jmax) * 8;
    const dim3 grid(B), block(64 * CN_WAVES);
    switch ((C + 63) / 64) {
        case 1: hipLaunchKernelGGL(ctc_confnet_kernel<1>, grid, block, lds, st, a); break;
        case 2: hipLaunchKernelGGL(ctc_confnet_kernel<2>, grid, block, lds, st, a); break;
        case 3: hipLaunchKernelGGL(ctc_confnet_kernel<3>, grid, block, lds, st, a); break;
        default: hipLaunchKernelGGL(ctc_confnet_kernel<4>, grid, block, lds, st, a); break;
    }
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { set_error("ctc confnet kernel launch failed: %s", hipGetErrorString(le)); return MDD_ERR_HIP; }
    return MDD_OK;
}
