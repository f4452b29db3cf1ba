// CTC prefix beam search, the generic kernel: any beam <= 64 and C <= 256, one workgroup of one wave per utterance (the reference, the
// pre-pass and the host path: beam.hip; the single-wave kernel for beam <= 16, C <= 64: beam_fast.hip).
#include "beam.h"

namespace mdd {

struct BeamMeta {       // one entry of `last` (BeamSearch.py:9-15); prefix bytes live in a separate LDS array
    double prTotal, prNonBlank, prBlank;
    unsigned long long hash, phash;  // rolling hash of the prefix and of the prefix without its last symbol
    int len, last;
};

// ---- pass 2: one wave per utterance, serial over the live frames.  dynamic LDS layout (bytes):
//   tot[beam*C] double | lmt[(C+1)*(C+1)] double (if it fits) | cl_v[beam*C] double | cl_o[beam*C] int |
//   flags[Tcap] uint8 | prefix[2][beam][Tcap] uint8
// NBEST selects the ending: false writes the winner alone (mdd_beam; nbest is 0), true the `nbest` best final hypotheses (mdd_beam_nbest).
template <bool NBEST>
__global__ __launch_bounds__(64) void beam_kernel(const double *__restrict__ lpw, const unsigned char *__restrict__ flags,
                                                  int T, int B, int C, const int32_t *__restrict__ len, int beam, int blank,
                                                  const double *__restrict__ lm, double alpha, int32_t *__restrict__ ids,
                                                  int32_t *__restrict__ nids, int32_t *__restrict__ status,
                                                  double *__restrict__ score, int Tcap, int lm_in_lds, int nbest) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int C1 = C + 1;
    double *tot = reinterpret_cast<double *>(sm);
    double *lmt = tot + (size_t)beam * C;
    double *cl_v = lmt + (lm_in_lds ? C1 * C1 : 0);                  // compacted candidate list (values)
    int *cl_o = reinterpret_cast<int *>(cl_v + (size_t)beam * C);    //   and their insertion orders
    unsigned char *fl = reinterpret_cast<unsigned char *>(cl_o + (size_t)beam * C);  // per-frame flags of this utterance [Tcap]
    unsigned char *pref = fl + Tcap;
    __shared__ double lp[256];
    __shared__ int nlist;
    __shared__ BeamMeta meta[2][MAXBEAM];
    __shared__ double cNB[MAXBEAM], cB[MAXBEAM], cT[MAXBEAM];  // copy-path contributions per beam
    __shared__ int parent[MAXBEAM], mslot[MAXBEAM];             // parent beam index / ext slot merged with this beam's copy
    __shared__ double sel_v[MAXBEAM];
    __shared__ int sel_ord[MAXBEAM];

    const int b = blockIdx.x, lane = threadIdx.x;
    int cur = 0, nb = 1, err = 0;
    if (lane == 0) {
        BeamMeta &m = meta[0][0];
        m.prTotal = 0.0; m.prBlank = 0.0; m.prNonBlank = LOG_ZERO; m.len = 0; m.last = -1;
        m.hash = BEAM_HASH_EMPTY; m.phash = 0;
    }
    if (lm_in_lds) for (int i = lane; i < C1 * C1; i += 64) lmt[i] = lm[i];
    const double *lmp = lm_in_lds ? lmt : lm;
    __syncthreads();
    int tl = len[b];
    tl = tl < 0 ? 0 : (tl > T ? T : tl);
    for (int i = lane; i < tl; i += 64) fl[i] = flags[(size_t)i * B + b];
    __syncthreads();

    // software prefetch: the row of the next live frame is loaded while the current one is processed
    int t = 0;
    while (t < tl && !(fl[t] & 1)) t++;
    double pre[4];
#pragma unroll
    for (int i = 0; i < 4; i++) pre[i] = (t < tl && lane + 64 * i < C) ? lpw[((size_t)t * B + b) * C + lane + 64 * i] : 0.0;
    while (t < tl) {
        const bool rep_ok = (fl[t] & 2) != 0;
#pragma unroll
        for (int i = 0; i < 4; i++) if (lane + 64 * i < C) lp[lane + 64 * i] = pre[i];
        int tn = t + 1;
        while (tn < tl && !(fl[tn] & 1)) tn++;
#pragma unroll
        for (int i = 0; i < 4; i++) pre[i] = (tn < tl && lane + 64 * i < C) ? lpw[((size_t)tn * B + b) * C + lane + 64 * i] : 0.0;
        __syncthreads();
        const BeamMeta *last = meta[cur];
        unsigned char *pcur = pref + (size_t)cur * beam * Tcap, *pnext = pref + (size_t)(cur ^ 1) * beam * Tcap;

        // ---- candidate scores.  slot idx = r*C + k ; k == blank is beam r's own ("copy") entry.
        // lanes own the class index k (k = lane, lane+64, ..), the beam rank r is a uniform loop.
        int first_err_ord = 0x7fffffff, first_err = 0;
        for (int r = 0; r < nb; r++) {
            const BeamMeta &y = last[r];
            const int ylen = y.len, ylast = y.last;
            const double yB = y.prBlank, yT = y.prTotal;
            const double *lmrow = lmp + (ylen ? ylast : C) * C1;
            for (int k = lane; k < C; k += 64) {
                if (k == blank) continue;
                const double lmv = lmrow[k];  // consulted even when alpha == 0 (:57-60)
                const double lk = lp[k];
                const int ord = r * C1 + 1 + k;
                if (lmv != lmv) { if (ord < first_err_ord) { first_err_ord = ord; first_err = MDD_BEAM_KEY_ERROR; } }
                else if (lk == -INFINITY) { if (ord < first_err_ord) { first_err_ord = ord; first_err = MDD_BEAM_VALUE_ERROR; } }
                const double base = (ylen && ylast == k && rep_ok) ? yB : yT;  // :63-66
                tot[r * C + k] = lk + lmv * alpha + base;
            }
        }
        if (lane < nb) {
            const BeamMeta &y = last[lane];
            double pnb = LOG_ZERO;
            bool bad = (lp[blank] == -INFINITY);
            if (y.len > 0) { pnb = y.prNonBlank + lp[y.last]; bad = bad || (lp[y.last] == -INFINITY); }  // :103
            const double pb = y.prTotal + lp[blank];                                                      // :106
            if (bad) { const int ord = lane * C1; if (ord < first_err_ord) { first_err_ord = ord; first_err = MDD_BEAM_VALUE_ERROR; } }
            cNB[lane] = pnb; cB[lane] = pb;
            const double tc = log_add_prob(pb, pnb);                                                      // :112
            cT[lane] = tc;
            tot[lane * C + blank] = tc;
            // parent candidate: a beam q whose (length, hash) equal those of y without its last symbol
            int par = -1;
            if (y.len > 0)
                for (int q = 0; q < nb; q++)
                    if (q != lane && last[q].len == y.len - 1 && last[q].hash == y.phash) { par = q; break; }
            parent[lane] = par;
            mslot[lane] = -1;
        }
        // verify the content of every hash match with the whole wave (a hash collision must never merge two
        // distinct prefixes): 64 lanes compare 64 words per pass, the tail word is masked to the prefix length
        for (int a = 0; a < nb; a++) {
            const int q = parent[a];          // uniform (LDS broadcast; written by lane a above, same wave, in order)
            if (q < 0) continue;
            const int ln = last[q].len;
            const unsigned int *wa = reinterpret_cast<const unsigned int *>(pcur + (size_t)a * Tcap);
            const unsigned int *wq = reinterpret_cast<const unsigned int *>(pcur + (size_t)q * Tcap);
            bool neq = false;
            for (int j = lane; j * 4 < ln; j += 64) {
                unsigned int x = wa[j] ^ wq[j];
                const int rem = ln - j * 4;
                if (rem < 4) x &= (1u << (8 * rem)) - 1u;
                neq = neq || (x != 0);
            }
            if (__any(neq) && lane == 0) parent[a] = -1;
        }
        {   // first error in the reference's execution order wins
            int eo = first_err_ord;
            for (int o = 32; o > 0; o >>= 1) eo = min(eo, __shfl_xor(eo, o));
            if (eo != 0x7fffffff) {
                const unsigned long long who = __ballot(first_err_ord == eo);
                err = __shfl(first_err, __ffsll((long long)who) - 1);
                break;
            }
        }
        __syncthreads();
        // ---- merges: beam a's copy entry and its parent's extension by a's last symbol are one dict entry
        int nmerge = 0;
        if (lane < nb && parent[lane] >= 0) {
            const int a = lane, q = parent[a], e = q * C + last[a].last;
            const double pr = tot[e];
            if (q < a) {  // entry was created by the extension (inserted earlier), then the copy is added (:108-113)
                cNB[a] = log_add_prob(pr, cNB[a]);
                cT[a] = log_add_prob(pr, cT[a]);
                tot[e] = cT[a];
                tot[a * C + blank] = -INFINITY;
                mslot[a] = e;
            } else {      // entry was created by the copy, then the extension is added (:122-125)
                cNB[a] = log_add_prob(cNB[a], pr);
                cT[a] = log_add_prob(cT[a], pr);
                tot[a * C + blank] = cT[a];
                tot[e] = -INFINITY;
            }
            nmerge = 1;
        }
        nmerge = __popcll(__ballot(nmerge != 0));
        __syncthreads();
        // ---- `last.sort()[0:beam]`: stable, descending by prTotal; insertion order = (r, copy first, then k ascending)
        const int ncand = nb * C - nmerge;
        const int keep = ncand < beam ? ncand : beam;
        // Top-`keep` of the <= nb*C candidates under (value desc, insertion order asc) without serial pops:
        //  1. theta0 = keep-th largest of the 64 per-lane maxima (rank counting over v_readlane broadcasts); at
        //     least `keep` candidates are >= theta0, so every member of the true top-`keep` is too;
        //  2. the few candidates >= theta0 are compacted into an LDS list (order irrelevant);
        //  3. each list entry counts the entries that beat it; rank < keep -> it IS output position `rank`.
        // insertion order of slot (r,k): r*C + (k == blank ? 0 : (k < blank ? k+1 : k)).
        const float invC = 1.0f / (float)C;
        auto idx_of = [&](int ord) {
            const int r = (int)(((float)ord + 0.5f) * invC), j = ord - r * C;
            return r * C + (j == 0 ? blank : (j <= blank ? j - 1 : j));
        };
        double lmax = -INFINITY;
        for (int r = 0; r < nb; r++)
            for (int k = lane; k < C; k += 64) lmax = fmax(lmax, tot[r * C + k]);
        int rk = 0;
        {
            const int lo = __double2loint(lmax), hi = __double2hiint(lmax);
#pragma unroll 8
            for (int j = 0; j < 64; j++) {
                const double sj = __hiloint2double(__builtin_amdgcn_readlane(hi, j), __builtin_amdgcn_readlane(lo, j));
                rk += (sj > lmax || (sj == lmax && j < lane)) ? 1 : 0;
            }
        }
        const unsigned long long mk = __ballot(rk == keep - 1);
        const int srcl = __ffsll((long long)mk) - 1;
        const double theta0 = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(lmax), srcl),
                                               __builtin_amdgcn_readlane(__double2loint(lmax), srcl));
        if (lane == 0) nlist = 0;
        __syncthreads();
        if (lmax >= theta0) {
            int cnt = 0;
            for (int r = 0; r < nb; r++)
                for (int k = lane; k < C; k += 64) cnt += (tot[r * C + k] >= theta0) ? 1 : 0;
            int pos = atomicAdd(&nlist, cnt);
            for (int r = 0; r < nb; r++)
                for (int k = lane; k < C; k += 64) {
                    const double v = tot[r * C + k];
                    if (v >= theta0) { cl_v[pos] = v; cl_o[pos] = beam_slot_order(r, k, C, blank); pos++; }
                }
        }
        __syncthreads();
        const int nl = nlist;
        for (int e = lane; e < nl; e += 64) {
            const double v = cl_v[e];
            const int o = cl_o[e];
            int rank = 0;
            for (int f = 0; f < nl; f++) {
                const double vf = cl_v[f];
                const int of = cl_o[f];
                rank += (vf > v || (vf == v && of < o)) ? 1 : 0;
            }
            if (rank < keep) { sel_v[rank] = v; sel_ord[rank] = idx_of(o); }
        }
        __syncthreads();
        // ---- materialise the new beams
        BeamMeta *next = meta[cur ^ 1];
        if (lane < keep) {
            const int idx = sel_ord[lane];
            const int r = (int)(((float)idx + 0.5f) * invC), k = idx - r * C;
            const BeamMeta &y = last[r];
            BeamMeta n;
            if (k == blank) {
                n.prTotal = sel_v[lane]; n.prNonBlank = cNB[r]; n.prBlank = cB[r];
                n.len = y.len; n.last = y.last; n.hash = y.hash; n.phash = y.phash;
            } else {
                n.prTotal = sel_v[lane]; n.prNonBlank = sel_v[lane]; n.prBlank = LOG_ZERO;
                for (int a = 0; a < nb; a++)
                    if (mslot[a] == idx) { n.prNonBlank = cNB[a]; n.prBlank = cB[a]; }
                n.len = y.len + 1; n.last = k; n.phash = y.hash;
                n.hash = beam_hash_push(y.hash, k);
            }
            next[lane] = n;
        }
        for (int i = 0; i < keep; i++) {
            const int idx = sel_ord[i];
            const int r = (int)(((float)idx + 0.5f) * invC), k = idx - r * C;
            const int ln = last[r].len;
            const unsigned int *src = reinterpret_cast<const unsigned int *>(pcur + (size_t)r * Tcap);
            unsigned int *dst = reinterpret_cast<unsigned int *>(pnext + (size_t)i * Tcap);
            for (int j = lane; j * 4 < ln; j += 64) dst[j] = src[j];      // Tcap % 4 == 0: whole words
            __builtin_amdgcn_wave_barrier();
            if (k != blank && lane == 0) reinterpret_cast<unsigned char *>(dst)[ln] = (unsigned char)k;
        }
        __syncthreads();
        cur ^= 1;
        nb = keep;
        t = tn;
    }
    __syncthreads();
    if constexpr (NBEST) {
        // ---- final, N best: EOS LM term and length normalisation per entry (thread r = entry r of `BHat`), the first failing entry
        // in entry order decides the status, then the reference's second sort() (:29-33,148) as a rank count through LDS --
        // rank(r) = #{j : s_j > s_r or (s_j == s_r and j < r)}: descending, equal scores keep their entry order (Python's sort is
        // stable and `curr` is filled in BHat order).  sel_v / sel_ord are dead after the frame loop.
        const BeamMeta *last = meta[cur];
        const bool act = lane < nb && !err;
        int e = 0;
        double s = -INFINITY;
        if (act) {
            const BeamMeta &y = last[lane];
            if (y.len == 0) e = MDD_BEAM_INDEX_ERROR;                  // y[-1] on the empty tuple (:135)
            else {
                const double v = lmp[y.last * C1 + C];
                if (v != v) e = MDD_BEAM_KEY_ERROR;
                else s = beam_final_score(y.prTotal, v, alpha, y.len);
            }
        }
        const unsigned long long em = __ballot(e != 0);
        if (em) err = __shfl(e, __ffsll((long long)em) - 1);
        sel_v[lane] = s;                                                // entries >= nb: -inf
        sel_ord[lane] = -1;
        __syncthreads();
        int rank = 0;
        for (int j = 0; j < nb; j++) {
            const double sj = sel_v[j];
            rank += (sj > s || (sj == s && j < lane)) ? 1 : 0;
        }
        if (!err && lane < nb) sel_ord[rank] = lane;                    // a permutation of 0..nb-1
        __syncthreads();
        const unsigned char *rows = pref + (size_t)cur * beam * Tcap;
        for (int n = 0; n < nbest; n++) {
            const int r = (err || n >= nb) ? -1 : sel_ord[n];
            const size_t o = (size_t)n * B + b;
            int ln = 0;
            if (r >= 0) {
                ln = last[r].len;
                const unsigned char *src = rows + (size_t)r * Tcap;
                for (int j = lane; j < ln; j += 64) ids[o * T + j] = src[j];
            }
            if (lane == 0) { nids[o] = ln; score[o] = r >= 0 ? sel_v[r] : __builtin_nan(""); }
        }
        if (lane == 0) status[b] = err;
    } else
    // ---- final: EOS LM term, length normalisation, first maximum (:130-148)
    if (lane == 0) {
        const BeamMeta *last = meta[cur];
        int best = -1;
        double bestv = 0.0;
        for (int r = 0; r < nb && !err; r++) {
            const BeamMeta &y = last[r];
            if (y.len == 0) { err = MDD_BEAM_INDEX_ERROR; break; }   // y[-1] on the empty tuple (:135)
            const double v = lmp[y.last * C1 + C];
            if (v != v) { err = MDD_BEAM_KEY_ERROR; break; }
            const double pr = beam_final_score(y.prTotal, v, alpha, y.len);
            if (best < 0 || pr > bestv) { best = r; bestv = pr; }
        }
        status[b] = err;
        int n = 0;
        if (!err && best >= 0) {
            n = last[best].len;
            const unsigned char *src = pref + (size_t)cur * beam * Tcap + (size_t)best * Tcap;
            for (int j = 0; j < n; j++) ids[(size_t)b * T + j] = src[j];
        }
        nids[b] = n;
        if (score) score[b] = err ? __builtin_nan("") : bestv;
    }
}

// The two instantiations, named once: f(bool_constant<NBEST>) for the ending the plan asks for
template <class F> static void with_beam_generic(bool nbest, F f) {
    if (nbest) f(std::true_type{}); else f(std::false_type{});
}

int init_beam_generic_attributes() {
    for (const bool nbest : {false, true}) {
        hipError_t e = hipSuccess;
        with_beam_generic(nbest, [&](auto nb) {
            e = hipFuncSetAttribute((const void *)beam_kernel<decltype(nb)::value>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBeamGenericLdsMax);
        });
        MDD_HIP_CHECK(e);
    }
    return MDD_OK;
}

void launch_beam_generic(const BeamCall &c, const BeamPlan &p, const double *lpw, const unsigned char *flags) {
    with_beam_generic(p.nbest, [&](auto nb) {
        hipLaunchKernelGGL(beam_kernel<decltype(nb)::value>, dim3(c.B), dim3(64), p.smem, c.st, lpw, flags, c.T, c.B, c.C, c.len, c.beam, c.blank, c.lm,
                           c.alpha, c.ids, c.nids, c.status, c.score, p.Tcap, p.lm_in_lds, c.nbest);
    });
}

}  // namespace mdd
