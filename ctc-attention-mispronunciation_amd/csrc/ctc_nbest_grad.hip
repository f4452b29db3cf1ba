// MWER training (DESIGN.md "MWER training"): the tensor the expected-phoneme-error objective of an N-best list deposits on the log-probs,
//   grad[t,b,c] = sum_n coef[n,b] * g_n[t,b,c],   g_n = exp(lp) - sum_{s: l'_s = c} exp(alpha_t(s) + beta_t(s) - ll_n - lp)
// (g_n: what mdd_ctc_loss deposits for hypothesis n as target), in ONE call -- where the parent's entries need N mdd_ctc_loss calls, each
// staging the utterance's log-probs again and writing a full [T,B,C] tensor, and N scaled additions.  mdd_nbest_risk beside it turns the
// list's log-likelihoods and costs into the posteriors, the risk and those coefficients.
//
// ctc_nbest_grad_kernel -- grid (groups of ranks, B); a workgroup of eight waves takes one utterance b and `ranks` consecutive ranks
// (plan.h, ctc_nbest_grad_plan):
//   * all its threads stage logp[0:Tb, b, :] into LDS once and clear an accumulator acc [Tb][C] fp32 beside it;
//   * ranks in ascending order.  A rank with coef == 0 is skipped by the whole workgroup (every thread reads the same coef: the trip
//     count and the barriers are the workgroup's, not a wave's).  For a live rank every wave reads the labels into registers and votes on
//     their range before any is an index; then wave 0 runs alpha, wave 1 beta, side by side, wave 2 builds the per-class lists of label
//     positions -- ctc_wave_kernel's (ctc.hip) three roles restated step for step, the rows going to the workgroup's slice of the
//     workspace, reused from rank to rank; after one barrier all waves turn frames into occupancy rows (the blank by wave_sum_dpp, the
//     labels by the per-class list walk) and subtract coef * occupancy from acc.  Frame t is wave t % 8's and class c lane c % 64's at
//     every rank: an accumulator element has ONE owner, so it needs no barrier and no atomic, and its additions come in ascending rank;
//   * the exp(lp) term is added once, as exp(lp) * sum_n coef (the sum in fp64, ascending n);
//   * with one group the workgroup stores  exp(lp) * S + acc  itself; with several each stores acc as a partial slab [T,B,C] into the
//     workspace and ctc_nbest_grad_sum_kernel adds the slabs in ascending group order -- the same expression with the slab sum for acc.
// Deterministic: no floating-point atomic, fixed orders throughout; the plan reads no switch.
// loglik: the alpha scan is ctc_nbest_kernel's (ctc_nbest.hip), so a scanned rank's value has the bits of mdd_ctc_nbest's.
// With N = 1 and coef = 1 the stored value is fexp(lp) * 1.f + (0.f - occupancy): the bits of mdd_ctc_loss's gradient.
#include "ctc_host.h"
#include "ctc_lse.h"
#include "ctc_wave.h"

namespace mdd {
namespace {

struct CtcNbestGradArgs {
    const float *logp; int T, B, C;
    const int32_t *len, *ids; int pitch; const int32_t *nids;
    int N, max_len, blank, ranks, groups;
    const double *coef;
    double *loglik;      // nullable
    float *grad;
    int32_t *flag;
    double *rows;        // [groups * B][2][T][SP]: alpha rows then beta rows of the workgroup's current rank
    int SP;              // row pitch in doubles = 2 * (max_len + 1)
    float *slabs;        // [groups][T][B][C], groups > 1 only
    int32_t *gflag;      // [groups][B], groups > 1 only
};

constexpr int kGradThreads = 64 * kCtcNbestGradWaves;

__device__ __forceinline__ double minus_nan() { return __longlong_as_double((long long)0xfff8000000000000ull); }

// dynamic LDS: lpt[T][C] f32 | acc[T][C] f32 | lab[LC] i32 | cls_off[C+1] i32 | cls_idx[LC] i32 | gam[8][LC] f32   (LC = 64 * NL)
template <int NL>
__global__ __launch_bounds__(kGradThreads) void ctc_nbest_grad_kernel(CtcNbestGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    constexpr int LC = 64 * NL;
    const int T = a.T, B = a.B, C = a.C, blank = a.blank;
    float *lpt = reinterpret_cast<float *>(sm);
    float *acc = lpt + (size_t)T * C;
    int *lab_s = reinterpret_cast<int *>(acc + (size_t)T * C);
    int *cls_off = lab_s + LC;
    int *cls_idx = cls_off + C + 1;
    float *gam = reinterpret_cast<float *>(cls_idx + LC);
    __shared__ double s_fin[2];
    const int b = blockIdx.y, grp = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int Tb = a.len[b];
    if (Tb > T) Tb = T;
    if (Tb < 0) Tb = 0;
    for (int e = tid; e < Tb * C; e += kGradThreads) {
        const int t = e / C, c = e - t * C;
        lpt[e] = a.logp[((size_t)t * B + b) * C + c];
        acc[e] = 0.f;
    }
    const bool direct = a.groups == 1;
    if (direct)   // padded frames carry zero gradient
        for (int e = Tb * C + tid; e < T * C; e += kGradThreads) {
            const int t = e / C, c = e - t * C;
            a.grad[((size_t)t * B + b) * C + c] = 0.f;
        }
    __syncthreads();         // the staged block and the cleared accumulator, also where no rank below is live
    double *wsa = a.rows + ((size_t)grp * B + b) * 2 * T * a.SP;
    double *wsb = wsa + (size_t)T * a.SP;
    float *g = gam + wave * LC;
    const int first = grp * a.ranks;
    const int last = first + a.ranks < a.N ? first + a.ranks : a.N;
    int flag = 0;            // the same value in every thread: it is made of values every thread reads alike
    double S = 0.0;          // sum of the coefficients, ascending n (the direct form; the several-group form sums them in the second kernel)
    for (int n = first; n < last; n++) {
        const double coef = a.coef[(size_t)n * B + b];
        double *ll_out = a.loglik ? a.loglik + (size_t)n * B + b : nullptr;
        if (coef == 0.0) {   // not scanned, whatever its ids are
            if (ll_out && tid == 0) *ll_out = __builtin_nan("");
            continue;
        }
        if (!(fabs(coef) <= 1.79769313486231570815e308)) flag = 2;     // inf or NaN
        S += coef;
        int L = a.nids[(size_t)n * B + b];
        if (L > a.max_len) L = a.max_len;
        if (L < 0) L = 0;
        // labels straight into registers, in every wave alike; lanes past the row's length hold the blank and read nothing
        const int32_t *row_ids = a.ids + ((size_t)n * B + b) * a.pitch;
        int lab[NL];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < NL; j++) {
            const int i = lane * NL + j;
            int l = blank;
            if (i < L) {
                const int v = row_ids[i];
                if (v < 0 || v >= C) bad = true; else l = v;
            }
            lab[j] = l;
        }
        const bool any_bad = __any(bad);
        if (any_bad || Tb == 0) {      // mdd_ctc_nbest's values: NaN for a label that would index past the row, 0 / -inf without frames
            if (ll_out && tid == 0) *ll_out = any_bad ? minus_nan() : (L == 0 ? -0.0 : -INFINITY);
            if (any_bad) flag = 2; else if (L > 0 && flag == 0) flag = 1;
            continue;
        }
        __syncthreads();     // the rank before this one is done with the rows, the lists and s_fin
        if (wave == 0) {
            // ---------------- alpha, forwards (ctc_wave_kernel's wave 0; the values of ctc_nbest_kernel's scan)
            bool skip[NL], valid_o[NL];
            const int left_lab = __shfl_up(lab[NL - 1], 1);
#pragma unroll
            for (int j = 0; j < NL; j++) {
                const int i = lane * NL + j;
                const int prev = j == 0 ? left_lab : lab[j - 1];
                valid_o[j] = i < L;
                skip[j] = i >= 1 && i < L && lab[j] != prev && lab[j] != blank;
            }
            double ae[NL], ao[NL];
            float lpb = lpt[blank], lpl[NL];
#pragma unroll
            for (int j = 0; j < NL; j++) lpl[j] = lpt[lab[j]];
#pragma unroll
            for (int j = 0; j < NL; j++) {
                const int i = lane * NL + j;
                ae[j] = i == 0 ? (double)lpb : -INFINITY;
                ao[j] = (i == 0 && L > 0) ? (double)lpl[j] : -INFINITY;
            }
            float nb = 0.f, nl[NL];
            if (Tb > 1) {
                const float *row = lpt + C;
                nb = row[blank];
#pragma unroll
                for (int j = 0; j < NL; j++) nl[j] = row[lab[j]];
            }
            for (int t = 0;; t++) {
                if (flag == 0) {
#pragma unroll
                    for (int j = 0; j < NL; j++) {
                        const int i = lane * NL + j;
                        if (i <= L) *reinterpret_cast<double2 *>(wsa + (size_t)t * a.SP + 2 * i) = make_double2(ae[j], ao[j]);
                    }
                }
                if (t + 1 >= Tb) break;
                lpb = nb;
#pragma unroll
                for (int j = 0; j < NL; j++) lpl[j] = nl[j];
                if (t + 2 < Tb) {
                    const float *row = lpt + (size_t)(t + 2) * C;
                    nb = row[blank];
#pragma unroll
                    for (int j = 0; j < NL; j++) nl[j] = row[lab[j]];
                }
                const double from_left = wave_shift<DPP_WAVE_SHR1>(ao[NL - 1]);
                double ne[NL], no[NL];
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    const double pol = j == 0 ? from_left : ao[j - 1];
                    ne[j] = wlse2(ae[j], pol) + (double)lpb;
                    no[j] = valid_o[j] ? wlse3(ao[j], ae[j], skip[j] ? pol : -INFINITY) + (double)lpl[j] : -INFINITY;
                }
#pragma unroll
                for (int j = 0; j < NL; j++) { ae[j] = ne[j]; ao[j] = no[j]; }
            }
            // log-likelihood: states 2L (blank behind the last label) and 2L-1 (the last label)
#pragma unroll
            for (int j = 0; j < NL; j++) {
                const int i = lane * NL + j;
                if (i == L) s_fin[0] = ae[j];
                if (i == L - 1) s_fin[1] = ao[j];
            }
            if (L == 0 && lane == 0) s_fin[1] = -INFINITY;
        } else if (wave == 1 && flag == 0) {
            // ---------------- beta, backwards (ctc_wave_kernel's wave 1)
            bool skip[NL];
            const int right_lab = __shfl_down(lab[0], 1);
#pragma unroll
            for (int j = 0; j < NL; j++) {
                const int i = lane * NL + j;
                const int next = j == NL - 1 ? right_lab : lab[j + 1];
                skip[j] = i + 1 < L && lab[j] != blank && lab[j] != next;
            }
            double be[NL], bo[NL];
            const float *row0 = lpt + (size_t)(Tb - 1) * C;
            float lpb = row0[blank], lpl[NL];
#pragma unroll
            for (int j = 0; j < NL; j++) lpl[j] = row0[lab[j]];
#pragma unroll
            for (int j = 0; j < NL; j++) {
                const int i = lane * NL + j;
                be[j] = i == L ? (double)lpb : -INFINITY;
                bo[j] = (i == L - 1) ? (double)lpl[j] : -INFINITY;
            }
            float nb = 0.f, nl[NL];
            if (Tb > 1) {
                const float *row = lpt + (size_t)(Tb - 2) * C;
                nb = row[blank];
#pragma unroll
                for (int j = 0; j < NL; j++) nl[j] = row[lab[j]];
            }
            for (int t = Tb - 1;; t--) {
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    const int i = lane * NL + j;
                    if (i <= L) *reinterpret_cast<double2 *>(wsb + (size_t)t * a.SP + 2 * i) = make_double2(be[j], bo[j]);
                }
                if (t == 0) break;
                lpb = nb;
#pragma unroll
                for (int j = 0; j < NL; j++) lpl[j] = nl[j];
                if (t >= 2) {
                    const float *row = lpt + (size_t)(t - 2) * C;
                    nb = row[blank];
#pragma unroll
                    for (int j = 0; j < NL; j++) nl[j] = row[lab[j]];
                }
                const double er = wave_shift<DPP_WAVE_SHL1>(be[0]), orr = wave_shift<DPP_WAVE_SHL1>(bo[0]);
                double ne[NL], no[NL];
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    const double ner = j == NL - 1 ? er : be[j + 1], nor_ = j == NL - 1 ? orr : bo[j + 1];
                    ne[j] = wlse2(be[j], bo[j]) + (double)lpb;
                    no[j] = wlse3(bo[j], ner, skip[j] ? nor_ : -INFINITY) + (double)lpl[j];
                }
#pragma unroll
                for (int j = 0; j < NL; j++) { be[j] = ne[j]; bo[j] = no[j]; }
            }
        } else if (wave == 2 && flag == 0) {
            // ---------------- per-class lists of label positions (ascending), for the deterministic class sums
#pragma unroll
            for (int j = 0; j < NL; j++) lab_s[lane * NL + j] = lab[j];
            wave_lds_order();
            for (int c = lane; c < C; c += 64) {
                int k = 0;
                for (int i = 0; i < L; i++) k += lab_s[i] == c;
                cls_off[c + 1] = k;
            }
            if (lane == 0) cls_off[0] = 0;
            wave_lds_order();
            if (lane == 0) for (int c = 0; c < C; c++) cls_off[c + 1] += cls_off[c];
            wave_lds_order();
            for (int c = lane; c < C; c += 64) {
                int k = cls_off[c];
                for (int i = 0; i < L; i++) if (lab_s[i] == c) cls_idx[k++] = i;
            }
        }
        __syncthreads();
        const double ll = wlse2(s_fin[0], s_fin[1]);
        if (ll_out && tid == 0) *ll_out = ll;
        if (ll == -INFINITY && flag == 0) flag = 1;       // no CTC path of the frames
        if (flag) continue;                               // the utterance's rows will be zeros: only the log-likelihoods go on
        // ---------------- acc -= coef * occupancy, all waves, frames dealt round-robin: frame t is wave t % 8's at every rank
        const float kf = (float)coef;
        for (int t = wave; t < Tb; t += kCtcNbestGradWaves) {
            const float *row = lpt + (size_t)t * C;
            const float lpb = row[blank];
            float ge = 0.f;
#pragma unroll
            for (int j = 0; j < NL; j++) {
                const int i = lane * NL + j;
                float go = 0.f;
                if (i <= L) {
                    const double2 al = *reinterpret_cast<const double2 *>(wsa + (size_t)t * a.SP + 2 * i);
                    const double2 be = *reinterpret_cast<const double2 *>(wsb + (size_t)t * a.SP + 2 * i);
                    ge += fexp((float)(al.x + be.x - ll - (double)lpb));
                    if (i < L) go = fexp((float)(al.y + be.y - ll - (double)row[lab[j]]));
                }
                g[lane * NL + j] = go;
            }
            const float gblank = wave_sum_dpp(ge);
            wave_lds_order();     // the walk below sees this frame's values
            for (int c = lane; c < C; c += 64) {
                float occ = c == blank ? gblank : 0.f;
                for (int k = cls_off[c]; k < cls_off[c + 1]; k++) occ += g[cls_idx[k]];
                acc[(size_t)t * C + c] -= kf * occ;
            }
            wave_lds_order();
        }
    }
    // ---------------- the rows of this workgroup, each by the wave and lane that own it
    if (direct) {
        if (tid == 0) a.flag[b] = flag;
        const float Sf = (float)S;
        for (int t = wave; t < Tb; t += kCtcNbestGradWaves)
            for (int c = lane; c < C; c += 64)
                a.grad[((size_t)t * B + b) * C + c] = flag ? 0.f : fexp(lpt[(size_t)t * C + c]) * Sf + acc[(size_t)t * C + c];
    } else {
        if (tid == 0) a.gflag[(size_t)grp * B + b] = flag;
        float *slab = a.slabs + (size_t)grp * T * B * C;
        for (int t = wave; t < Tb; t += kCtcNbestGradWaves)
            for (int c = lane; c < C; c += 64) slab[((size_t)t * B + b) * C + c] = acc[(size_t)t * C + c];
    }
}

// The several-group form's second half: grid (ceil(T * C / 256), B).  flag[b] is the largest of the groups' flags; an element is
// exp(lp) * S + (slab 0 + slab 1 + ..), the slabs in ascending group order, S the fp64 sum of the live coefficients in ascending n.
__global__ __launch_bounds__(256) void ctc_nbest_grad_sum_kernel(CtcNbestGradArgs a) {
    const int T = a.T, B = a.B, C = a.C, b = blockIdx.y;
    int Tb = a.len[b];
    if (Tb > T) Tb = T;
    if (Tb < 0) Tb = 0;
    int flag = 0;
    for (int gq = 0; gq < a.groups; gq++) { const int f = a.gflag[(size_t)gq * B + b]; flag = f > flag ? f : flag; }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.flag[b] = flag;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= T * C) return;
    const int t = e / C, c = e - t * C;
    const size_t at = ((size_t)t * B + b) * C + c;
    if (flag || t >= Tb) { a.grad[at] = 0.f; return; }
    double S = 0.0;
    for (int n = 0; n < a.N; n++) S += a.coef[(size_t)n * B + b];      // a skipped rank's coefficient is 0
    float sum = a.slabs[at];
    for (int gq = 1; gq < a.groups; gq++) sum += a.slabs[(size_t)gq * T * B * C + at];
    a.grad[at] = fexp(a.logp[at]) * (float)S + sum;
}

template <int NL> int ctc_nbest_grad_set_lds() {
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)ctc_nbest_grad_kernel<NL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCtcNbestGradLdsMax));
    return MDD_OK;
}
int init_ctc_nbest_grad_attributes() {
    if (int rc = ctc_nbest_grad_set_lds<1>()) return rc;
    if (int rc = ctc_nbest_grad_set_lds<2>()) return rc;
    return ctc_nbest_grad_set_lds<4>();
}

template <int NL> void launch_ctc_nbest_grad(const CtcNbestGradArgs &a, const CtcNbestGradPlan &p, hipStream_t st) {
    hipLaunchKernelGGL(ctc_nbest_grad_kernel<NL>, dim3(p.groups, a.B), dim3(kGradThreads), p.smem, st, a);
}

struct RiskArgs {
    const double *loglik; const int32_t *cost, *status; int N, B;
    double *post, *risk, *coef; int32_t *flag;
};

__device__ __forceinline__ double risk_wave_sum(double v) {      // __shfl_xor over distances 32, 16, .., 1: every lane the same bits (mbr.hip's)
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ bool risk_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// One wave per utterance; lanes take ranks lane, lane + 64, .. in ascending order, then a butterfly: fixed orders, the same bits on every call.
__global__ __launch_bounds__(64) void nbest_risk_kernel(RiskArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x, N = a.N, B = a.B;
    double m = -INFINITY;
    bool neg = false;
    for (int n = lane; n < N; n += 64) {
        const double v = a.loglik[(size_t)n * B + b];
        if (risk_finite(v)) m = fmax(m, v);
        neg = neg || a.cost[(size_t)n * B + b] < 0;
    }
    for (int o = 32; o; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    const bool skipped = a.status && a.status[b] != 0;
    const int flag = skipped ? 1 : __any(neg) ? 2 : m == -INFINITY ? 1 : 0;
    if (lane == 0) a.flag[b] = flag;
    if (flag) {
        for (int n = lane; n < N; n += 64) { a.post[(size_t)n * B + b] = 0.0; a.coef[(size_t)n * B + b] = 0.0; }
        if (lane == 0) a.risk[b] = __builtin_nan("");
        return;
    }
    double z = 0.0;
    for (int n = lane; n < N; n += 64) {
        const double v = a.loglik[(size_t)n * B + b];
        if (risk_finite(v)) z += exp(v - m);
    }
    z = risk_wave_sum(z);
    double r = 0.0;
    for (int n = lane; n < N; n += 64) {
        const double v = a.loglik[(size_t)n * B + b];
        const double p = risk_finite(v) ? exp(v - m) / z : 0.0;
        a.post[(size_t)n * B + b] = p;
        r += p * (double)a.cost[(size_t)n * B + b];
    }
    r = risk_wave_sum(r);
    if (lane == 0) a.risk[b] = r;
    for (int n = lane; n < N; n += 64) {
        const double v = a.loglik[(size_t)n * B + b];
        const double p = risk_finite(v) ? exp(v - m) / z : 0.0;
        a.coef[(size_t)n * B + b] = p * (r - (double)a.cost[(size_t)n * B + b]);
    }
}

const char *ctc_nbest_grad_shape_error(int T, int B, int C, int N, int max_len, int pitch, int blank) {
    return (N < 1 || N > kCtcNbestMaxN) ? "need 1<=N<=256" : (B < 1 || B > 65535) ? "need 1<=B<=65535" : (C < 2 || C > 256) ? "need 2<=C<=256"
         : T < 1 ? "T < 1" : (blank < 0 || blank >= C) ? "blank outside [0, C)"
         : (max_len < 0 || max_len > kCtcNbestMaxLen || max_len > pitch) ? "need 0<=max_len<=min(pitch, 255)"
         : !ctc_nbest_grad_fits(T, C, max_len) ? "T too long for LDS: see mdd_ctc_nbest_grad_fits" : nullptr;
}

}  // namespace
}  // namespace mdd

using namespace mdd;

extern "C" int mdd_ctc_nbest_grad_fits(int32_t T, int32_t C, int32_t max_len) { return ctc_nbest_grad_fits(T, C, max_len) ? 1 : 0; }

extern "C" int64_t mdd_ctc_nbest_grad_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t N, int32_t max_len) {
    if (ctc_nbest_grad_shape_error(T, B, C, N, max_len, max_len, 0)) return 0;
    return (int64_t)ctc_nbest_grad_plan(T, B, C, N, max_len).bytes;
}

// In the order of ctc_host.h: refuse, attributes, workspace, launch, check.
extern "C" int mdd_ctc_nbest_grad(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, const int32_t *ids_dev, int32_t pitch,
                                  const int32_t *nids_dev, int32_t N, int32_t max_len, int32_t blank, const double *coef_dev, double *loglik_dev,
                                  float *grad_dev, int32_t *flag_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    const char *what = !logp_dev ? "logp_dev is NULL" : !len_dev ? "len_dev is NULL" : !ids_dev ? "ids_dev is NULL" : !nids_dev ? "nids_dev is NULL"
                     : !coef_dev ? "coef_dev is NULL" : !grad_dev ? "grad_dev is NULL" : !flag_dev ? "flag_dev is NULL"
                     : ctc_nbest_grad_shape_error(T, B, C, N, max_len, pitch, blank);
    if (what) { set_error("mdd_ctc_nbest_grad: bad argument (%s)", what); return MDD_ERR_ARG; }
    const CtcNbestGradPlan p = ctc_nbest_grad_plan(T, B, C, N, max_len);
    if (workspace_dev && workspace_bytes < (int64_t)p.bytes)
        return refuse_workspace("mdd_ctc_nbest_grad", "mdd_ctc_nbest_grad_workspace_bytes", workspace_bytes, (int64_t)p.bytes);
    hipStream_t st = (hipStream_t)stream;
    static OncePerDevice once;
    if (int rc = once_per_device(once, init_ctc_nbest_grad_attributes)) return rc;
    StreamWorkspace ws;
    if (int rc = ws.acquire(workspace_dev, (int64_t)p.bytes, st)) return rc;
    unsigned char *base = ws.as<unsigned char>();
    CtcNbestGradArgs a{logp_dev, T, B, C, len_dev, ids_dev, pitch, nids_dev, N, max_len, blank, p.ranks, p.groups, coef_dev, loglik_dev, grad_dev,
                       flag_dev, reinterpret_cast<double *>(base), p.SP, reinterpret_cast<float *>(base + p.rows_bytes),
                       reinterpret_cast<int32_t *>(base + p.rows_bytes + p.slab_bytes)};
    switch (p.NL) {
        case 1: launch_ctc_nbest_grad<1>(a, p, st); break;
        case 2: launch_ctc_nbest_grad<2>(a, p, st); break;
        default: launch_ctc_nbest_grad<4>(a, p, st); break;
    }
    if (p.groups > 1) hipLaunchKernelGGL(ctc_nbest_grad_sum_kernel, dim3((T * C + 255) / 256, B), dim3(256), 0, st, a);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { set_error("mdd_ctc_nbest_grad: kernel launch failed: %s", hipGetErrorString(le)); return MDD_ERR_HIP; }
    return MDD_OK;
}

extern "C" int mdd_nbest_risk(const double *loglik_dev, const int32_t *cost_dev, const int32_t *status_dev, int32_t N, int32_t B, double *post_dev,
                              double *risk_dev, double *coef_dev, int32_t *flag_dev, void *stream) {
    const char *what = !loglik_dev ? "loglik_dev is NULL" : !cost_dev ? "cost_dev is NULL" : !post_dev ? "post_dev is NULL" : !risk_dev ? "risk_dev is NULL"
                     : !coef_dev ? "coef_dev is NULL" : !flag_dev ? "flag_dev is NULL" : (N < 1 || N > kCtcNbestMaxN) ? "need 1<=N<=256"
                     : B < 1 ? "B < 1" : nullptr;
    if (what) { set_error("mdd_nbest_risk: bad argument (%s)", what); return MDD_ERR_ARG; }
    RiskArgs a{loglik_dev, cost_dev, status_dev, N, B, post_dev, risk_dev, coef_dev, flag_dev};
    hipLaunchKernelGGL(nbest_risk_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { set_error("mdd_nbest_risk: kernel launch failed: %s", hipGetErrorString(le)); return MDD_ERR_HIP; }
    return MDD_OK;
}
