// Per-phoneme CTC posteriors: the CTC log-likelihood of every sequence ONE edit away from the canonical ids -- every substitution
// y[i] -> k, every deletion of y[i], every insertion of k in gap g -- from the two lattices of the canonical sequence alone.
//
// No reference counterpart.  Formulas (DESIGN.md "One-edit variants"): states s = 0..2L, 2i the blank before label i, 2i+1 label i;
// alpha_t(s) / beta_t(s) the forward / backward log lattices of ctc.hip (both include the emission at t); (+) is log-add.
//   One label slot -- a new label k between the blank states sL and sR (substitution at i: sL = 2i, sR = 2i+2; insertion in gap g:
//   sL = sR = 2g); left = label of state sL-1, right = label of state sR+1, where those states exist:
//     in_0 = 0 if sL == 0 else -inf;       in_t = alpha_{t-1}(sL) (+) [left exists, left != k] alpha_{t-1}(sL-1)
//     gamma_t = (gamma_{t-1} (+) in_t) + lp[t,k],   gamma_{-1} = -inf
//     out_{T-1} = 0 if sR == 2L else -inf;  out_t = beta_{t+1}(sR) (+) [right exists, right != k] beta_{t+1}(sR+1)
//     logP = (+)_t (gamma_t + out_t)
//   Deletion of i -- no recurrence; skip = i >= 1 and i+1 < L and y[i-1] != y[i+1]:
//     i+1 < L:  (+)_{t < T-1} (alpha_t(2i) (+) [skip] alpha_t(2i-1)) + beta_{t+1}(2i+3);   i == L-1: alpha_{T-1}(2i) (and alpha_{T-1}(2i-1), i >= 1);
//     i == 0 and L > 1: beta_0(3).
//
// Phase 1: ctc.hip's scan on the int32 ids (ctc_lattice): both rows of every frame in an fp64 workspace.
// Phase 2, ctc_variants_head_kernel: a wave per utterance screens the ids and writes base and status, once.
// Phase 3, ctc_variants_kernel: a wave per slot (L substitution rows, L+1 insertion rows), lanes over k, a second pass over the frames
//   for classes 64.. when C > 64.  A slot's chains differ only in k, so the four lattice values of a step (alpha_{t-1}(sL), alpha_{t-1}(sL-1),
//   beta_{t+1}(sR), beta_{t+1}(sR+1)) are uniform over the wave: both forms of in_t and out_t are computed once for all lanes and a lane
//   picks its own.  They and the row lp[t, :] (coalesced) are requested one step ahead of their use, so the dependent chain of a step is
//   one log-add and one addition (gamma).  In a substitution slot the lane k == blank sums the deletion instead (the same uniform
//   values, one step apart) and the lane k == ids[i] copies base; in an insertion slot the lane k == blank copies base.
//   Four slots share a workgroup, one wave per SIMD: the waves share nothing (no LDS, no barrier).  Measured at B = 64, T = 250, C = 45,
//   L = 64 (profiles/ctc_variants_notes.txt): 1, 2 or 4 slots per workgroup time alike, 8 is 5 % slower; the phase scales with the slot
//   count (8 waves per SIMD at that shape), i.e. it is bound by the four log-adds of a step, not by the latency of one chain.
//   Log-adds as in ctc.hip (ctc_lse.h).  No atomics: the same bits on every call.
#include <math.h>
#include <stdlib.h>

#include "ctc_host.h"
#include "ctc_lse.h"

namespace mdd {

static constexpr int VAR_WAVES = 4;       // slots per workgroup: one wave per SIMD (MDD_CTC_VARIANTS_WAVES = 1, 2, 4 or 8 overrides it, for timing)
static constexpr int VAR_WAVES_MAX = 8;

struct VariantArgs {
    const float *logp; int T, B, C;
    const int *len, *ids; int ids_stride;
    const int *nids; int Lmax, blank;
    double *base, *sub, *ins; int *status;
    CtcLattice lat;
    int nslots, nblk;   // slots per utterance, workgroups per utterance
};

// Once per utterance, a wave each: the target check, base and status.  The slots below read both back, so the ids are screened once
// and not once per slot.
__global__ __launch_bounds__(64) void ctc_variants_head_kernel(VariantArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int C = a.C, blank = a.blank;
    int Tb = a.len[b];
    if (Tb > a.T) Tb = a.T;
    if (Tb < 0) Tb = 0;
    int L = a.nids[b];
    bool bad = L < 0 || L > a.Lmax;
    if (bad) L = 0;
    const int *ids = a.ids + (size_t)b * a.ids_stride;
    bool mine = false;
    for (int i = lane; i < L; i += 64) { const int v = ids[i]; mine |= v < 0 || v >= C || v == blank; }
    bad = bad || __any(mine);
    // log P(canonical): states 2L and 2L-1 of the last frame, combined as ctc.hip combines them
    double base;
    if (bad) base = NAN;
    else if (Tb == 0) base = L == 0 ? 0.0 : -INFINITY;
    else {
        const double *last = a.lat.alpha + (size_t)b * a.lat.utt_stride + (size_t)(Tb - 1) * a.lat.pitch;
        base = wlse2(last[2 * L], L > 0 ? last[2 * L - 1] : -INFINITY);
    }
    if (lane == 0) {
        a.base[b] = base;
        a.status[b] = bad ? MDD_ALIGN_BAD_TARGET : (base == -INFINITY ? MDD_ALIGN_INFEASIBLE : MDD_ALIGN_OK);
    }
}

__global__ __launch_bounds__(64 * VAR_WAVES_MAX) void ctc_variants_kernel(VariantArgs a) {
    const int b = blockIdx.x / a.nblk;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int slot = (blockIdx.x - b * a.nblk) * (int)(blockDim.x >> 6) + wave;
    if (slot >= a.nslots) return;
    const int B = a.B, C = a.C, blank = a.blank, Lmax = a.Lmax;
    int Tb = a.len[b];
    if (Tb > a.T) Tb = a.T;
    if (Tb < 0) Tb = 0;
    const bool bad = a.status[b] == MDD_ALIGN_BAD_TARGET;      // ctc_variants_head_kernel's verdict
    const double base = a.base[b];
    const int L = bad ? 0 : a.nids[b];
    const int *ids = a.ids + (size_t)b * a.ids_stride;
    const double *al = a.lat.alpha + (size_t)b * a.lat.utt_stride, *be = a.lat.beta + (size_t)b * a.lat.utt_stride;
    const size_t pitch = (size_t)a.lat.pitch;
    const bool is_sub = slot < Lmax;
    const int row = is_sub ? slot : slot - Lmax;
    if (!is_sub && !a.ins) return;
    double *out = is_sub ? a.sub + ((size_t)b * a.ids_stride + row) * C : a.ins + ((size_t)b * (a.ids_stride + 1) + row) * C;
    const bool pad = is_sub ? row >= L : row > L;
    const int own = (is_sub && !bad && !pad) ? ids[row] : -1;
    if (bad || pad || Tb == 0) {
        for (int k = lane; k < C; k += 64) {
            double v = bad ? NAN : -INFINITY;
            if (!bad && !pad) {     // no frames: only the empty sequence has an alignment
                if (is_sub) v = k == blank ? (L == 1 ? 0.0 : -INFINITY) : (k == own ? base : -INFINITY);
                else v = k == blank ? base : -INFINITY;
            }
            out[k] = v;
        }
        return;
    }
    const int sL = 2 * row, sR = is_sub ? 2 * row + 2 : 2 * row;
    const int left = row >= 1 ? ids[row - 1] : -1;                                              // label of state sL-1
    const int right = is_sub ? (row + 1 < L ? ids[row + 1] : -1) : (row < L ? ids[row] : -1);   // label of state sR+1
    const bool has_l = left >= 0, has_r = right >= 0;
    const bool del_mid = is_sub && row + 1 < L, del_skip = del_mid && row >= 1 && left != right;
    const double in0 = sL == 0 ? 0.0 : -INFINITY, out_last = sR == 2 * L ? 0.0 : -INFINITY;
    const float *lp_b = a.logp + (size_t)b * C;
    const size_t lp_step = (size_t)B * C;
    for (int k0 = 0; k0 < C; k0 += 64) {
        const int k = k0 + lane;
        const int kk = k < C ? k : C - 1;      // lanes past the last class run a chain nobody reads
        const bool use_l = has_l && left != kk, use_r = has_r && right != kk;
        const bool is_del = is_sub && kk == blank;
        double g = -INFINITY, acc = -INFINITY;
        // n*: the values of the next step, requested while this step computes
        float nlp = lp_b[kk];
        double naL = -INFINITY, naL1 = -INFINITY, nbR = -INFINITY, nbR1 = -INFINITY;
        if (Tb > 1) {
            nbR = be[pitch + sR];
            if (has_r) nbR1 = be[pitch + sR + 1];
        }
        double b_prev = -INFINITY;      // beta_t(sR+1), for the deletion term of frame t-1
        for (int t = 0; t < Tb; t++) {
            const float lp = nlp;
            const double aL = naL, aL1 = naL1, bR = nbR, bR1 = nbR1;
            if (t + 1 < Tb) {
                nlp = lp_b[(size_t)(t + 1) * lp_step + kk];
                naL = al[(size_t)t * pitch + sL];
                if (has_l) naL1 = al[(size_t)t * pitch + sL - 1];
                if (t + 2 < Tb) {
                    nbR = be[(size_t)(t + 2) * pitch + sR];
                    if (has_r) nbR1 = be[(size_t)(t + 2) * pitch + sR + 1];
                }
            }
            const double in_both = wlse2(aL, aL1), out_both = wlse2(bR, bR1);       // uniform over the wave
            const double in_t = t == 0 ? in0 : (use_l ? in_both : aL);
            const double out_t = t == Tb - 1 ? out_last : (use_r ? out_both : bR);
            g = wlse2(g, in_t) + (double)lp;
            double term = g + out_t;
            if (is_del) term = (del_mid && t >= 1) ? (del_skip ? in_both : aL) + b_prev : -INFINITY;
            acc = wlse2(acc, term);
            b_prev = bR1;
        }
        if (is_del) {
            const double *last = al + (size_t)(Tb - 1) * pitch;
            if (row == L - 1) {
                acc = wlse2(acc, last[2 * row]);
                if (row >= 1) acc = wlse2(acc, last[2 * row - 1]);
            }
            if (row == 0 && L > 1) acc = wlse2(acc, be[3]);
        }
        const bool copy = is_sub ? kk == own : kk == blank;
        if (k < C) out[k] = copy ? base : acc;
    }
}

}  // namespace mdd

extern "C" int64_t mdd_ctc_variants_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t Lmax) {
    if (T <= 0 || B <= 0 || C <= 0 || Lmax < 0) return 0;
    return mdd::ctc_lattice_bytes(T, B, C, Lmax);
}

extern "C" int mdd_ctc_variants(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, const int32_t *ids_dev,
                                int32_t ids_stride, const int32_t *nids_dev, int32_t Lmax, int32_t blank, double *base_dev, double *sub_dev,
                                double *ins_dev, int32_t *status_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    using namespace mdd;
    const char *what = !logp_dev ? "logp_dev is NULL" : !len_dev ? "len_dev is NULL" : !ids_dev ? "ids_dev is NULL" : !nids_dev ? "nids_dev is NULL"
                     : !base_dev ? "base_dev is NULL" : !sub_dev ? "sub_dev is NULL" : !status_dev ? "status_dev is NULL" : T <= 0 ? "T <= 0"
                     : B <= 0 ? "B <= 0" : C <= 0 ? "C <= 0" : C > 256 ? "C > 256" : (blank < 0 || blank >= C) ? "blank outside [0, C)"
                     : Lmax < 0 ? "Lmax < 0" : Lmax > ids_stride ? "Lmax > ids_stride" : !ctc_lattice_fits(T, C, Lmax) ? "Lmax too long for LDS" : nullptr;
    if (what) { set_error("mdd_ctc_variants: %s", what); return MDD_ERR_ARG; }
    const int64_t need = mdd_ctc_variants_workspace_bytes(T, B, C, Lmax);
    if (workspace_dev && workspace_bytes < need) return refuse_workspace("mdd_ctc_variants", "mdd_ctc_variants_workspace_bytes", workspace_bytes, need);
    VariantArgs a;
    a.nslots = Lmax + (ins_dev ? Lmax + 1 : 0);
    int waves = VAR_WAVES;
    if (const char *e = getenv("MDD_CTC_VARIANTS_WAVES")) { const int w = atoi(e); if (w == 1 || w == 2 || w == 4 || w == 8) waves = w; }
    a.nblk = (a.nslots + waves - 1) / waves;
    if ((int64_t)B * a.nblk > 0x7fffffffLL) { set_error("mdd_ctc_variants: B x Lmax too large for one launch"); return MDD_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    StreamWorkspace ws;
    if (int rc = ws.acquire(workspace_dev, need, st)) return rc;
    if (int rc = ctc_lattice(logp_dev, T, B, C, len_dev, ids_dev, ids_stride, nids_dev, Lmax, blank, ws.as<double>(), st, &a.lat)) return rc;
    hipError_t le = hipGetLastError();
    if (le == hipSuccess) {
        a.logp = logp_dev; a.T = T; a.B = B; a.C = C; a.len = len_dev; a.ids = ids_dev; a.ids_stride = ids_stride; a.nids = nids_dev;
        a.Lmax = Lmax; a.blank = blank; a.base = base_dev; a.sub = sub_dev; a.ins = ins_dev; a.status = status_dev;
        hipLaunchKernelGGL(ctc_variants_head_kernel, dim3(B), dim3(64), 0, st, a);
        if (a.nslots > 0) hipLaunchKernelGGL(ctc_variants_kernel, dim3((unsigned)(B * a.nblk)), dim3(64 * waves), 0, st, a);
        le = hipGetLastError();
    }
    if (le != hipSuccess) { set_error("ctc variants kernel launch failed: %s", hipGetErrorString(le)); return MDD_ERR_HIP; }
    return MDD_OK;
}
