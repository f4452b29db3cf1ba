// CTC forced alignment: the max-product (Viterbi) form of the lattice in ctc.hip, with a traceback.
//
// No reference counterpart (the reference diagnoses by edit distance only).  One pass serves two products: aligning the DECODED ids
// gives every decoded phoneme a start frame, an end frame and a confidence; aligning the CANONICAL ids gives every canonical phoneme
// the mean log-posterior over the frames the model would have to give it (goodness of pronunciation).
//
// Arithmetic (DESIGN.md "Forced alignment"): states s = 0..2L are blank, label 0, blank, ..., label L-1, blank; values fp32.
//   v[0][0] = lp[0][blank], v[0][1] = lp[0][ids[0]], -inf elsewhere;   v[t][s] = best + lp[t][label(s)]  (ONE fp32 addition),
//   best over v[t-1][s] (stay), v[t-1][s-1], and v[t-1][s-2] for a label state whose label differs from the label two states back.
//   Ties: stay wins over s-1, s-1 wins over s-2 -- a move is taken only on strict '>'.  The path ends in state 2L only if
//   v[2L] > v[2L-1] strictly, else in 2L-1 (L = 0: state 0).  seg_logp[i] is summed in fp32 in ascending frame order.
// No transcendental function and no reduction of variable order: both kernels below and a float32 loop on the host give the same bits.
// fp32 and not the loss's fp64: a max-product path is a plain sum of T' log-probs (no log-add whose error grows with the magnitude of
// the values), and fp32 is what makes the bit-exact restatement possible.
//
// ctc_align_wave_kernel -- ctc_wave_kernel's layout: one workgroup per utterance, wave 0 scans; a lane owns NL consecutive labels,
//   each with the blank state in front of it (the lane with i == L owns the closing blank); one DPP wave shift per step brings the
//   left neighbour's last label state; the log-probs are staged in LDS and requested one step ahead; the only LDS traffic in the
//   dependent chain is the backpointer store (2 bits per state = one nibble per label slot, next to the staged log-probs).  Lane 0
//   then walks the backpointers (T' dependent LDS reads) into a path row in LDS, and the whole workgroup turns that row into
//   path / seg / seg_logp: a thread per frame finds the segment edges, a thread per label sums its own frames in time order.
//   LDS: T x C x 4 (log-probs) + T x 64 x max(NL, 2) / 2 (backpointers) + T x 4 (path) + 64 x NL x 12 (labels, segment edges).
// ctc_align_generic_kernel -- a thread per four states, value rows in LDS, one barrier per frame, backpointers (2 bits per state),
//   path row and segment edges in the workspace; any Lmax the rows fit LDS for, any T, any C.  Same bits as the wave form.
#include <stdlib.h>
#include <string.h>

#include "ctc_host.h"
#include "ctc_wave.h"

namespace mdd {

static constexpr size_t ALIGN_LDS_LIMIT = 150 * 1024;

struct AlignArgs {
    const float *logp; int T, B, C;
    const int *len, *ids; int ids_stride;
    const int *nids; int Lmax, blank;
    float *score; int *status, *path, *seg; float *seg_logp;
    unsigned char *ws;      // generic form only
    long long ws_utt;       // bytes per utterance
    int S4;                 // generic form: groups of four states per row = ceil((2 Lmax + 1) / 4)
};

// Path row -> outputs, by the whole workgroup (every thread must arrive).  path[t] for t < Tb (read only when ok), edges: 2 x Lmax ints
// of scratch; lp(t, c) = lp[t * lp_stride + c]; the label of position i is lab[i * lab_step + lab_off].
__device__ __forceinline__ void align_outputs(const AlignArgs &a, int b, int Tb, bool ok, const int *path, int *edges, const float *lp,
                                              size_t lp_stride, const int *lab, int lab_step, int lab_off) {
    const int tid = threadIdx.x, nth = blockDim.x, T = a.T;
    const bool want_seg = a.seg != nullptr;
    if (want_seg)
        for (int i = tid; i < 2 * a.Lmax; i += nth) edges[i] = -1;
    __syncthreads();
    for (int t = tid; t < T; t += nth) {
        const int pv = (ok && t < Tb) ? path[t] : -1;
        if (a.path) a.path[(size_t)b * T + t] = pv;
        if (want_seg && pv >= 0) {
            if (t == 0 || path[t - 1] != pv) edges[2 * pv] = t;
            if (t == Tb - 1 || path[t + 1] != pv) edges[2 * pv + 1] = t + 1;
        }
    }
    __syncthreads();
    if (want_seg)
        for (int i = tid; i < a.Lmax; i += nth) {
            const int s = edges[2 * i], e = edges[2 * i + 1];
            float acc = 0.f;
            if (s >= 0) {
                const int c = lab[i * lab_step + lab_off];
                acc = lp[(size_t)s * lp_stride + c];
                for (int t = s + 1; t < e; t++) acc += lp[(size_t)t * lp_stride + c];
            }
            const size_t o = (size_t)b * a.ids_stride + i;
            a.seg[2 * o] = s;
            a.seg[2 * o + 1] = e;
            a.seg_logp[o] = acc;
        }
}

// bytes of backpointers per frame in the wave form: a nibble per label slot, at least a byte per lane
__host__ __device__ constexpr int align_bp_pitch(int NL) { return NL == 1 ? 64 : 32 * NL; }

static size_t align_wave_smem(int T, int C, int NL) {
    const size_t LC = 64 * (size_t)NL;
    return (size_t)T * C * 4 + LC * 4 + (size_t)T * 4 + 2 * LC * 4 + (size_t)T * align_bp_pitch(NL);
}

// dynamic LDS: lpt[T][C] f32 | lab[LC] i32 | path[T] i32 | edges[2 LC] i32 | bp[T][pitch] u8      (LC = 64 * NL)
template <int NL>
__global__ __launch_bounds__(256) void ctc_align_wave_kernel(AlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    constexpr int LC = 64 * NL, PITCH = align_bp_pitch(NL);
    const int T = a.T, B = a.B, C = a.C, blank = a.blank;
    float *lpt = reinterpret_cast<float *>(sm);
    int *lab_s = reinterpret_cast<int *>(lpt + (size_t)T * C);
    int *path_s = lab_s + LC;
    int *edges = path_s + T;
    unsigned char *bp = reinterpret_cast<unsigned char *>(edges + 2 * LC);
    __shared__ float s_fin[2];
    __shared__ int s_bad, s_ok;
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int Tb = a.len[b], L = a.nids[b];
    if (Tb > T) Tb = T;
    if (Tb < 0) Tb = 0;
    const bool bad_len = L < 0 || L > a.Lmax;
    if (bad_len) L = 0;
    if (tid == 0) { s_bad = bad_len ? 1 : 0; s_ok = 0; }
    __syncthreads();
    for (int i = tid; i < LC; i += blockDim.x) {
        int l = blank;
        if (i < L) {
            const int v = a.ids[(size_t)b * a.ids_stride + i];
            if (v < 0 || v >= C || v == blank) s_bad = 1; else l = v;
        }
        lab_s[i] = l;
    }
    for (int e = tid; e < Tb * C; e += blockDim.x) {
        const int t = e / C, c = e - t * C;
        lpt[e] = a.logp[((size_t)t * B + b) * C + c];
    }
    __syncthreads();
    const bool bad = s_bad != 0;
    if (bad || Tb == 0) {
        if (tid == 0) {
            const bool ok = !bad && L == 0;
            a.score[b] = bad ? NAN : (ok ? 0.f : -INFINITY);
            a.status[b] = bad ? MDD_ALIGN_BAD_TARGET : (ok ? MDD_ALIGN_OK : MDD_ALIGN_INFEASIBLE);
        }
    } else if (wave == 0) {
        int lab[NL];
#pragma unroll
        for (int j = 0; j < NL; j++) lab[j] = lab_s[lane * NL + j];
        bool skip[NL], valid_o[NL];
        const int left_lab = __shfl_up(lab[NL - 1], 1);
#pragma unroll
        for (int j = 0; j < NL; j++) {
            const int i = lane * NL + j;
            const int prev = j == 0 ? left_lab : lab[j - 1];
            valid_o[j] = i < L;
            skip[j] = i >= 1 && i < L && lab[j] != prev;
        }
        float ae[NL], ao[NL];
        float lpb = lpt[blank], lpl[NL];
#pragma unroll
        for (int j = 0; j < NL; j++) lpl[j] = lpt[lab[j]];
#pragma unroll
        for (int j = 0; j < NL; j++) {
            const int i = lane * NL + j;
            ae[j] = i == 0 ? lpb : -INFINITY;
            ao[j] = (i == 0 && L > 0) ? lpl[j] : -INFINITY;
        }
        // lpb / lpl hold row t's log-probs while row t is computed; row t+1's are requested first (ctc_wave_kernel)
        float nb = 0.f, nl[NL];
#pragma unroll
        for (int j = 0; j < NL; j++) nl[j] = 0.f;
        if (Tb > 1) {
            const float *row = lpt + C;
            nb = row[blank];
#pragma unroll
            for (int j = 0; j < NL; j++) nl[j] = row[lab[j]];
        }
        for (int t = 1; t < Tb; t++) {
            lpb = nb;
#pragma unroll
            for (int j = 0; j < NL; j++) lpl[j] = nl[j];
            if (t + 1 < Tb) {
                const float *row = lpt + (size_t)(t + 1) * C;
                nb = row[blank];
#pragma unroll
                for (int j = 0; j < NL; j++) nl[j] = row[lab[j]];
            }
            const float from_left = wave_shift<DPP_WAVE_SHR1>(ao[NL - 1]);
            float ne[NL], no[NL];
            unsigned moves = 0;
#pragma unroll
            for (int j = 0; j < NL; j++) {
                const float pol = j == 0 ? from_left : ao[j - 1];       // state 2i-1: the previous label
                float be = ae[j];
                unsigned me = 0;
                if (pol > be) { be = pol; me = 1; }
                ne[j] = be + lpb;
                float bo = ao[j];
                unsigned mo = 0;
                if (ae[j] > bo) { bo = ae[j]; mo = 1; }
                if (skip[j] && pol > bo) { bo = pol; mo = 2; }
                no[j] = valid_o[j] ? bo + lpl[j] : -INFINITY;
                moves |= (me | (mo << 2)) << (4 * j);
            }
#pragma unroll
            for (int j = 0; j < NL; j++) { ae[j] = ne[j]; ao[j] = no[j]; }
            if (NL <= 2) bp[(size_t)t * PITCH + lane] = (unsigned char)moves;
            else *reinterpret_cast<unsigned short *>(bp + (size_t)t * PITCH + 2 * lane) = (unsigned short)moves;
        }
        // states 2L (the closing blank) and 2L-1 (the last label)
#pragma unroll
        for (int j = 0; j < NL; j++) {
            const int i = lane * NL + j;
            if (i == L) s_fin[0] = ae[j];
            if (i == L - 1) s_fin[1] = ao[j];
        }
        wave_lds_order();
        if (lane == 0) {
            const float f0 = s_fin[0], f1 = L > 0 ? s_fin[1] : -INFINITY;
            const bool last_blank = L == 0 || f0 > f1;
            const float sc = last_blank ? f0 : f1;
            const bool ok = sc != -INFINITY;
            a.score[b] = sc;
            a.status[b] = ok ? MDD_ALIGN_OK : MDD_ALIGN_INFEASIBLE;
            s_ok = ok ? 1 : 0;
            if (ok) {
                int s = last_blank ? 2 * L : 2 * L - 1;
                for (int t = Tb - 1;; t--) {
                    path_s[t] = (s & 1) ? (s >> 1) : -1;
                    if (t == 0) break;
                    const int i = s >> 1;       // label slot: blank 2i in bits 0-1 of its nibble, label 2i+1 in bits 2-3
                    const unsigned nib = NL == 1 ? bp[(size_t)t * PITCH + i] : (bp[(size_t)t * PITCH + (i >> 1)] >> (4 * (i & 1)));
                    s -= (nib >> (2 * (s & 1))) & 3;
                }
            }
        }
    }
    __syncthreads();
    align_outputs(a, b, Tb, s_ok != 0, path_s, edges, lpt, (size_t)C, lab_s, 1, 0);
}

// dynamic LDS: row[2][4 S4] f32 | lab[4 S4] i32.   workspace per utterance: bp[T][S4] u8 (16-byte padded) | path[T] i32 | edges[2 Lmax] i32
__global__ __launch_bounds__(256) void ctc_align_generic_kernel(AlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int T = a.T, B = a.B, C = a.C, blank = a.blank, S4 = a.S4, SP = 4 * S4;
    float *row = reinterpret_cast<float *>(sm);     // [2][SP]
    int *lab = reinterpret_cast<int *>(row + 2 * SP);
    __shared__ int s_bad, s_ok;
    const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    int Tb = a.len[b], L = a.nids[b];
    if (Tb > T) Tb = T;
    if (Tb < 0) Tb = 0;
    const bool bad_len = L < 0 || L > a.Lmax;
    if (bad_len) L = 0;
    const int S = 2 * L + 1;
    unsigned char *bp = a.ws + (size_t)b * a.ws_utt;
    int *path_w = reinterpret_cast<int *>(bp + (((size_t)T * S4 + 15) & ~(size_t)15));
    int *edges = path_w + T;
    if (tid == 0) { s_bad = bad_len ? 1 : 0; s_ok = 0; }
    __syncthreads();
    for (int s = tid; s < SP; s += nth) {
        int l = blank;
        if ((s & 1) && s < S) {
            const int v = a.ids[(size_t)b * a.ids_stride + (s >> 1)];
            if (v < 0 || v >= C || v == blank) s_bad = 1; else l = v;
        }
        lab[s] = l;
    }
    __syncthreads();
    const bool bad = s_bad != 0;
    const float *lp = a.logp + (size_t)b * C;
    const size_t lp_stride = (size_t)B * C;
    if (bad || Tb == 0) {
        if (tid == 0) {
            const bool ok = !bad && L == 0;
            a.score[b] = bad ? NAN : (ok ? 0.f : -INFINITY);
            a.status[b] = bad ? MDD_ALIGN_BAD_TARGET : (ok ? MDD_ALIGN_OK : MDD_ALIGN_INFEASIBLE);
        }
    } else {
        for (int s = tid; s < SP; s += nth) {
            row[s] = s == 0 ? lp[blank] : ((s == 1 && L > 0) ? lp[lab[1]] : -INFINITY);
            row[SP + s] = -INFINITY;
        }
        __syncthreads();
        for (int t = 1; t < Tb; t++) {
            const float *prev = row + ((t - 1) & 1) * SP;
            float *curr = row + (t & 1) * SP;
            const float *lpr = lp + (size_t)t * lp_stride;
            for (int g = tid; g < S4; g += nth) {
                unsigned moves = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int s = 4 * g + k;
                    if (s >= S) break;
                    const int l = lab[s];
                    float best = prev[s];
                    unsigned m = 0;
                    if (s >= 1 && prev[s - 1] > best) { best = prev[s - 1]; m = 1; }
                    if ((s & 1) && s >= 3 && l != lab[s - 2] && prev[s - 2] > best) { best = prev[s - 2]; m = 2; }
                    curr[s] = best + lpr[l];
                    moves |= m << (2 * k);
                }
                bp[(size_t)t * S4 + g] = (unsigned char)moves;
            }
            __syncthreads();
        }
        if (tid == 0) {
            const float *last = row + ((Tb - 1) & 1) * SP;
            const float f0 = last[S - 1], f1 = L > 0 ? last[S - 2] : -INFINITY;
            const bool last_blank = L == 0 || f0 > f1;
            const float sc = last_blank ? f0 : f1;
            const bool ok = sc != -INFINITY;
            a.score[b] = sc;
            a.status[b] = ok ? MDD_ALIGN_OK : MDD_ALIGN_INFEASIBLE;
            s_ok = ok ? 1 : 0;
            if (ok) {
                int s = last_blank ? 2 * L : 2 * L - 1;
                for (int t = Tb - 1;; t--) {
                    path_w[t] = (s & 1) ? (s >> 1) : -1;
                    if (t == 0) break;
                    s -= (bp[(size_t)t * S4 + (s >> 2)] >> (2 * (s & 3))) & 3;
                }
            }
        }
    }
    __syncthreads();
    align_outputs(a, b, Tb, s_ok != 0, path_w, edges, lp, lp_stride, lab, 2, 1);
}

static bool align_wave_form(int T, int C, int Lmax) {
    const char *e = getenv("MDD_CTC_ALIGN");
    return Lmax <= 255 && C <= 256 && align_wave_smem(T, C, ctc_labels_per_lane(Lmax)) <= ALIGN_LDS_LIMIT && !(e && !strcmp(e, "generic"));
}

static long long align_generic_ws_utt(int T, int Lmax) {
    const long long S4 = (2 * (long long)Lmax + 1 + 3) / 4;
    const long long n = (((long long)T * S4 + 15) & ~15LL) + 4LL * T + 8LL * Lmax;
    return (n + 15) & ~15LL;
}

static int init_align_attributes() {
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)ctc_align_wave_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ALIGN_LDS_LIMIT));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)ctc_align_wave_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ALIGN_LDS_LIMIT));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)ctc_align_wave_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ALIGN_LDS_LIMIT));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)ctc_align_generic_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ALIGN_LDS_LIMIT));
    return MDD_OK;
}

}  // namespace mdd

// bytes of workspace mdd_ctc_align needs for these shapes: 0 in the wave form, backpointers + path row + segment edges in the general form
extern "C" int64_t mdd_ctc_align_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t Lmax) {
    if (T <= 0 || B <= 0 || C <= 0 || Lmax < 0) return 0;
    if (mdd::align_wave_form(T, C, Lmax)) return 0;
    return (int64_t)B * mdd::align_generic_ws_utt(T, Lmax);
}

extern "C" int mdd_ctc_align(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, const int32_t *ids_dev,
                             int32_t ids_stride, const int32_t *nids_dev, int32_t Lmax, int32_t blank, float *score_dev,
                             int32_t *status_dev, int32_t *path_dev, int32_t *seg_dev, float *seg_logp_dev, void *workspace_dev,
                             int64_t workspace_bytes, void *stream) {
    using namespace mdd;
    const char *what = !logp_dev ? "logp_dev is NULL" : !len_dev ? "len_dev is NULL" : !ids_dev ? "ids_dev is NULL" : !nids_dev ? "nids_dev is NULL"
                     : !score_dev ? "score_dev is NULL" : !status_dev ? "status_dev is NULL" : T <= 0 ? "T <= 0" : B <= 0 ? "B <= 0"
                     : C <= 0 ? "C <= 0" : (blank < 0 || blank >= C) ? "blank outside [0, C)" : Lmax < 0 ? "Lmax < 0"
                     : Lmax > ids_stride ? "Lmax > ids_stride" : ((seg_dev == nullptr) != (seg_logp_dev == nullptr)) ? "seg_dev and seg_logp_dev must be given together"
                     : nullptr;
    if (what) { set_error("mdd_ctc_align: %s", what); return MDD_ERR_ARG; }
    const int64_t need = mdd_ctc_align_workspace_bytes(T, B, C, Lmax);
    if (workspace_dev && workspace_bytes < need) return refuse_workspace("mdd_ctc_align", "mdd_ctc_align_workspace_bytes", workspace_bytes, need);
    const bool wave_form = align_wave_form(T, C, Lmax);
    const int S4 = (2 * Lmax + 1 + 3) / 4;
    const size_t generic_smem = (size_t)48 * S4;
    if (!wave_form && generic_smem > ALIGN_LDS_LIMIT) { set_error("mdd_ctc_align: Lmax=%d too long for LDS", Lmax); return MDD_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    static OncePerDevice once;
    if (int rc = once_per_device(once, init_align_attributes)) return rc;
    StreamWorkspace ws;
    if (int rc = ws.acquire(workspace_dev, need, st)) return rc;
    AlignArgs a;
    a.logp = logp_dev; a.T = T; a.B = B; a.C = C; a.len = len_dev; a.ids = ids_dev; a.ids_stride = ids_stride; a.nids = nids_dev;
    a.Lmax = Lmax; a.blank = blank; a.score = score_dev; a.status = status_dev; a.path = path_dev; a.seg = seg_dev; a.seg_logp = seg_logp_dev;
    a.ws = ws.as<unsigned char>(); a.ws_utt = align_generic_ws_utt(T, Lmax); a.S4 = S4;
    if (wave_form) {
        const int NL = ctc_labels_per_lane(Lmax);
        const size_t smem = align_wave_smem(T, C, NL);
        if (NL == 1) hipLaunchKernelGGL(ctc_align_wave_kernel<1>, dim3(B), dim3(256), smem, st, a);
        else if (NL == 2) hipLaunchKernelGGL(ctc_align_wave_kernel<2>, dim3(B), dim3(256), smem, st, a);
        else hipLaunchKernelGGL(ctc_align_wave_kernel<4>, dim3(B), dim3(256), smem, st, a);
    } else {
        hipLaunchKernelGGL(ctc_align_generic_kernel, dim3(B), dim3(256), generic_smem, st, a);
    }
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { set_error("ctc align kernel launch failed: %s", hipGetErrorString(le)); return MDD_ERR_HIP; }
    return MDD_OK;
}
