// Rescoring an N-best list (mdd_ctc_nbest; DESIGN.md "N-best rescoring"): the exact CTC log-likelihood of every hypothesis of every
// utterance, ids [N,B,pitch] / nids [N,B] as the beam entries write them, in ONE launch -- where BeamDecoder.nbest_loglik made one
// mdd_ctc_loss call per rank, each staging the utterance's log-probs again and scanning on one wave of eight.
//
// ctc_nbest_kernel -- grid (groups of ranks, B); a workgroup takes one utterance b and hyps_per_block consecutive ranks (plan.h,
// ctc_nbest_plan):
//   * all its threads stage logp[0:Tb, b, :] into LDS once; ONE barrier; from there on the waves run on their own, wave w the ranks
//     first + w, first + w + waves, ..: the waves' trip counts differ (a partial last group, a wave with no rank), so nothing behind the
//     barrier may wait for another wave, and nothing does -- a wave's labels, lattice and result live in its registers;
//   * a scan is the alpha half of ctc_wave_kernel (ctc.hip) restated step for step: a lane owns NL consecutive labels and the blank state
//     in front of each (states 2i, 2i + 1), takes one value per step from its left neighbour by a DPP wave shift, adds in fp64 with fp32
//     increments (ctc_lse.h, the same operands in the same order) and requests a frame's two log-probs one step ahead of their use.
//     (float)(-loglik) therefore has the bits of mdd_ctc_loss's nll for the same row, which tests/test_ctc_nbest.py holds it to;
//   * a label outside [0, C) within a row's length is found by a wave vote before any label is an index: that (n, b) alone is NaN.
// No beta scan, no workspace, no gradient.
#include "ctc_host.h"
#include "ctc_lse.h"
#include "ctc_wave.h"

namespace mdd {
namespace {

struct CtcNbestArgs {
    const float *logp; int T, B, C;
    const int32_t *len, *ids; int pitch; const int32_t *nids;
    int N, max_len, blank, hyps_per_block;
    double *loglik;
};

constexpr int kCtcNbestMaxThreads = 64 * kCtcNbestMaxWaves;

// dynamic LDS: lpt[Tb][C] f32
template <int NL>
__global__ __launch_bounds__(kCtcNbestMaxThreads) void ctc_nbest_kernel(CtcNbestArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    float *lpt = reinterpret_cast<float *>(sm);
    const int T = a.T, B = a.B, C = a.C, blank = a.blank;
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nthreads = blockDim.x, nwave = nthreads >> 6;
    int Tb = a.len[b];
    if (Tb > T) Tb = T;
    if (Tb < 0) Tb = 0;
    // stage the utterance's log-probs: rows of C floats, B*C apart
    for (int e = tid; e < Tb * C; e += nthreads) {
        const int t = e / C, c = e - t * C;
        lpt[e] = a.logp[((size_t)t * B + b) * C + c];
    }
    __syncthreads();
    // ---------------- no workgroup barrier from here on: the waves run on their own
    const int first = blockIdx.x * a.hyps_per_block;
    const int last = first + a.hyps_per_block < a.N ? first + a.hyps_per_block : a.N;
    for (int n = first + wave; n < last; n += nwave) {
        int L = a.nids[(size_t)n * B + b];
        if (L > a.max_len) L = a.max_len;
        if (L < 0) L = 0;
        // labels straight into registers; lanes past the row's length hold the blank and read nothing
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
        double *out = a.loglik + (size_t)n * B + b;
        // the negated values of mdd_ctc_loss's nll: NaN for a label that would index past the row, 0 / +inf for an utterance without frames
        // (sign bits included: -NAN, so that the negation gives the float NAN the loss kernel stores)
        const bool any_bad = __any(bad);
        if (any_bad || Tb == 0) {
            if (lane == 0) *out = any_bad ? __longlong_as_double((long long)0xfff8000000000000ull) : (L == 0 ? -0.0 : -INFINITY);
            continue;
        }
        // ---------------- alpha, forwards (ctc_wave_kernel's wave 0)
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
        // lpb / lpl hold the log-probs of row t+1 while row t+1 is being computed; row t+2's are requested first, so their
        // LDS latency lies beside the step's arithmetic, not in front of it
        float nb = 0.f, nl[NL];
        if (Tb > 1) {
            const float *row = lpt + C;
            nb = row[blank];
#pragma unroll
            for (int j = 0; j < NL; j++) nl[j] = row[lab[j]];
        }
        for (int t = 0; t + 1 < Tb; t++) {
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
        // log-likelihood: states 2L (blank behind the last label) and 2L-1 (the last label), each from the lane that owns it
        double fe = -INFINITY, fo = -INFINITY;
#pragma unroll
        for (int j = 0; j < NL; j++) {
            const int i = lane * NL + j;
            if (i == L) fe = ae[j];
            if (i == L - 1) fo = ao[j];
        }
        fe = __shfl(fe, L / NL);
        fo = L > 0 ? __shfl(fo, (L - 1) / NL) : -INFINITY;
        if (lane == 0) *out = wlse2(fe, fo);
    }
}

template <int NL> int ctc_nbest_set_lds() {
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)ctc_nbest_kernel<NL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCtcNbestLdsMax));
    return MDD_OK;
}
int init_ctc_nbest_attributes() {
    if (int rc = ctc_nbest_set_lds<1>()) return rc;
    if (int rc = ctc_nbest_set_lds<2>()) return rc;
    return ctc_nbest_set_lds<4>();
}

template <int NL> void launch_ctc_nbest(const CtcNbestArgs &a, const CtcNbestPlan &p, hipStream_t st) {
    hipLaunchKernelGGL(ctc_nbest_kernel<NL>, dim3(p.groups, a.B), dim3(64 * p.waves), p.smem, st, a);
}

}  // namespace
}  // namespace mdd

using namespace mdd;

extern "C" int mdd_ctc_nbest_fits(int32_t T, int32_t C, int32_t max_len) { return ctc_nbest_fits(T, C, max_len) ? 1 : 0; }

// In the order of ctc_host.h: refuse, attributes, launch, check (the call has no workspace).
extern "C" int mdd_ctc_nbest(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, const int32_t *ids_dev, int32_t pitch,
                             const int32_t *nids_dev, int32_t N, int32_t max_len, int32_t blank, double *loglik_dev, void *stream) {
    const char *what = !logp_dev ? "logp_dev is NULL" : !len_dev ? "len_dev is NULL" : !ids_dev ? "ids_dev is NULL" : !nids_dev ? "nids_dev is NULL"
                     : !loglik_dev ? "loglik_dev is NULL" : (N < 1 || N > kCtcNbestMaxN) ? "need 1<=N<=256" : (B < 1 || B > 65535) ? "need 1<=B<=65535"
                     : (C < 2 || C > 256) ? "need 2<=C<=256" : T < 1 ? "T < 1" : (blank < 0 || blank >= C) ? "blank outside [0, C)"
                     : (max_len < 0 || max_len > kCtcNbestMaxLen || max_len > pitch) ? "need 0<=max_len<=min(pitch, 255)"
                     : !ctc_nbest_fits(T, C, max_len) ? "T too long for LDS: T*C*4 bytes past the 116 KiB of mdd_ctc_nbest_fits" : nullptr;
    if (what) { set_error("mdd_ctc_nbest: bad argument (%s)", what); return MDD_ERR_ARG; }
    const CtcNbestPlan p = ctc_nbest_plan(T, B, C, N, max_len, read_ctc_nbest_switches());
    hipStream_t st = (hipStream_t)stream;
    static OncePerDevice once;
    if (int rc = once_per_device(once, init_ctc_nbest_attributes)) return rc;
    CtcNbestArgs a{logp_dev, T, B, C, len_dev, ids_dev, pitch, nids_dev, N, max_len, blank, p.hyps_per_block, loglik_dev};
    switch (p.NL) {
        case 1: launch_ctc_nbest<1>(a, p, st); break;
        case 2: launch_ctc_nbest<2>(a, p, st); break;
        default: launch_ctc_nbest<4>(a, p, st); break;
    }
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { set_error("mdd_ctc_nbest: kernel launch failed: %s", hipGetErrorString(le)); return MDD_ERR_HIP; }
    return MDD_OK;
}
