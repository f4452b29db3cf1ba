// CTC prefix beam search, the wide kernel: any beam <= 256, C <= 256 and T <= 38400, one workgroup of eight waves per utterance (the
// reference and the pre-pass: beam.hip; the LDS budget, the workspace layout and the byte counts: plan.h, beam_wide_plan).
//
// The algorithm and its arithmetic are beam_generic.hip's, statement for statement where a number is computed (the copy and extension
// scores, log_add_prob, the two merge orders, beam_final_score), so every total is the same bits; what is selected is decided by the same
// total order (value descending, insertion order ascending), which has one answer however it is computed.  What differs is where the
// state lives and who does the work:
//   - per-beam state (2 x 256 entries) in static LDS; candidate totals and the compacted list in dynamic LDS while they fit, else in the
//     utterance's slice of the workspace; prefix rows (ping-pong, Tcap bytes each), the live-frame list, the pre-pass's log-probs and
//     flags in the workspace;
//   - candidates are dealt to the 512 threads by slot index (slot = r * C + k), not by class, so that the per-thread maxima of the
//     selection are spread over beams as well as classes; beams (copy entries, parent search, merges, new state) go one per thread;
//     prefix rows (content check, copy, output) one per wave.
#include <limits.h>

#include "beam.h"

namespace mdd {

constexpr int WB = kBeamWideMax, WT = kBeamWideThreads, WW = kBeamWideThreads / 64;
static_assert(WT >= WB && WT % 64 == 0, "the selection needs a maximum per beam to keep");

struct WideMeta {       // one entry of `last` (BeamSearch.py:9-15); its prefix bytes are a row of the workspace
    double prTotal, prNonBlank, prBlank;
    unsigned long long hash, phash;  // rolling hash of the prefix and of the prefix without its last symbol
    int len, last;
};

struct BeamWideArgs {
    const double *lpw; const unsigned char *flags;      // the pre-pass's outputs
    unsigned char *utt;                                  // the utterance slices, and inside one (beam_wide_plan):
    size_t utt_bytes, u_pref, u_tot, u_clv, u_clo;
    int T, B, C; const int32_t *len; int beam, blank; const double *lm; double alpha; int nbest;
    int32_t *ids, *nids, *status; double *score;
    int Tcap, list_cap;
};

// dynamic LDS: tot [beam*C] f64 (TOT_LDS) | cl_v [list_cap] f64 | cl_o [list_cap] i32
template <bool TOT_LDS>
__global__ __launch_bounds__(WT) void beam_wide_kernel(const BeamWideArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    __shared__ double lp[256];
    __shared__ WideMeta meta[2][WB];
    __shared__ double cNB[WB], cB[WB], cT[WB];        // copy-path contributions per beam
    __shared__ int parent[WB], mslot[WB];             // parent beam index / ext slot merged with this beam's copy
    __shared__ double sel_v[WB];
    __shared__ int sel_ord[WB];
    __shared__ double tmax[WT];                       // per-thread maxima of the selection
    __shared__ double theta_s;
    __shared__ int nlist, nmerge_s, errkey, endkey, wcount[WW];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, B = a.B, C = a.C, C1 = C + 1, beam = a.beam, blank = a.blank, Tcap = a.Tcap;
    const double alpha = a.alpha;
    const double *lmp = a.lm;
    unsigned char *slice = a.utt + (size_t)b * a.utt_bytes;
    int *live = reinterpret_cast<int *>(slice);
    unsigned char *pref = slice + a.u_pref;
    const size_t n = (size_t)beam * C;
    double *tot = TOT_LDS ? reinterpret_cast<double *>(sm) : reinterpret_cast<double *>(slice + a.u_tot);
    double *lcl_v = reinterpret_cast<double *>(sm) + (TOT_LDS ? n : 0);
    int *lcl_o = reinterpret_cast<int *>(lcl_v + a.list_cap);
    double *gcl_v = reinterpret_cast<double *>(slice + a.u_clv);     // read only where a list is longer than list_cap: the plan then has them
    int *gcl_o = reinterpret_cast<int *>(slice + a.u_clo);

    if (tid == 0) {
        WideMeta &m = meta[0][0];
        m.prTotal = 0.0; m.prBlank = 0.0; m.prNonBlank = LOG_ZERO; m.len = 0; m.last = -1;
        m.hash = BEAM_HASH_EMPTY; m.phash = 0;
        endkey = INT_MAX;
    }
    int tl = a.len[b];
    tl = tl < 0 ? 0 : (tl > T ? T : tl);
    // ---- the live frames of this utterance, in order: live[i] = t * 2 + (repeat bit of frame t)
    int nlive = 0;
    for (int base = 0; base < tl; base += WT) {
        const int t = base + tid;
        const unsigned char f = t < tl ? a.flags[(size_t)t * B + b] : 0;
        const bool lv = (f & 1) != 0;
        const unsigned long long m = __ballot(lv);
        if (lane == 0) wcount[wave] = __popcll(m);
        __syncthreads();
        int off = nlive, all = 0;
        for (int w = 0; w < WW; w++) { const int c = wcount[w]; off += w < wave ? c : 0; all += c; }
        if (lv) live[off + __popcll(m & ((1ull << lane) - 1ull))] = t * 2 + ((f >> 1) & 1);
        nlive += all;
        __syncthreads();
    }
    __syncthreads();

    int cur = 0, nb = 1, err = 0;
    // software prefetch: the row of the next live frame is loaded while the current one is processed, its index one frame earlier still
    int e0 = nlive > 0 ? live[0] : 0, e1 = nlive > 1 ? live[1] : 0;
    double pre = (nlive > 0 && tid < C) ? a.lpw[((size_t)(e0 >> 1) * B + b) * C + tid] : 0.0;
    const float invC = 1.0f / (float)C;
    for (int i = 0; i < nlive; i++) {
        const bool rep_ok = (e0 & 1) != 0;
        if (tid < C) lp[tid] = pre;
        const int e2 = i + 2 < nlive ? live[i + 2] : 0;
        pre = (i + 1 < nlive && tid < C) ? a.lpw[((size_t)(e1 >> 1) * B + b) * C + tid] : 0.0;
        if (tid == 0) { errkey = INT_MAX; nlist = 0; nmerge_s = 0; }
        __syncthreads();
        const WideMeta *last = meta[cur];
        unsigned char *pcur = pref + (size_t)cur * beam * Tcap, *pnext = pref + (size_t)(cur ^ 1) * beam * Tcap;
        const int nslot = nb * C;

        // ---- candidate scores.  slot idx = r*C + k ; k == blank is beam r's own ("copy") entry.
        // The first error is the smallest ord = r*C1 + (copy: 0, extension by k: 1 + k), the reference's execution order; key = ord*4 + code.
        int my_err = INT_MAX;
        for (int idx = tid; idx < nslot; idx += WT) {
            const int r = (int)(((float)idx + 0.5f) * invC), k = idx - r * C;
            if (k == blank) continue;
            const WideMeta &y = last[r];
            const int ylen = y.len, ylast = y.last;
            const double lmv = lmp[(ylen ? ylast : C) * C1 + k];  // consulted even when alpha == 0 (:57-60)
            const double lk = lp[k];
            const int ord = r * C1 + 1 + k;
            if (lmv != lmv) my_err = min(my_err, ord * 4 + MDD_BEAM_KEY_ERROR);
            else if (lk == -INFINITY) my_err = min(my_err, ord * 4 + MDD_BEAM_VALUE_ERROR);
            const double base = (ylen && ylast == k && rep_ok) ? y.prBlank : y.prTotal;  // :63-66
            tot[idx] = lk + lmv * alpha + base;
        }
        if (tid < nb) {
            const WideMeta &y = last[tid];
            double pnb = LOG_ZERO;
            bool bad = (lp[blank] == -INFINITY);
            if (y.len > 0) { pnb = y.prNonBlank + lp[y.last]; bad = bad || (lp[y.last] == -INFINITY); }  // :103
            const double pb = y.prTotal + lp[blank];                                                      // :106
            if (bad) my_err = min(my_err, tid * C1 * 4 + MDD_BEAM_VALUE_ERROR);
            cNB[tid] = pnb; cB[tid] = pb;
            const double tc = log_add_prob(pb, pnb);                                                      // :112
            cT[tid] = tc;
            tot[tid * C + blank] = tc;
            // parent candidate: a beam q whose (length, hash) equal those of y without its last symbol
            int par = -1;
            if (y.len > 0)
                for (int q = 0; q < nb; q++)
                    if (q != tid && last[q].len == y.len - 1 && last[q].hash == y.phash) { par = q; break; }
            parent[tid] = par;
            mslot[tid] = -1;
        }
        if (my_err != INT_MAX) atomicMin(&errkey, my_err);
        __syncthreads();
        if (errkey != INT_MAX) { err = errkey & 3; break; }   // first error in the reference's execution order wins
        // verify the content of every hash match, a wave per beam (a hash collision must never merge two distinct prefixes): 64 lanes
        // compare 64 words per pass, the tail word is masked to the prefix length
        for (int x = wave; x < nb; x += WW) {
            const int q = parent[x];
            if (q < 0) continue;
            const int ln = last[q].len;
            const unsigned int *wa = reinterpret_cast<const unsigned int *>(pcur + (size_t)x * Tcap);
            const unsigned int *wq = reinterpret_cast<const unsigned int *>(pcur + (size_t)q * Tcap);
            bool neq = false;
            for (int j = lane; j * 4 < ln; j += 64) {
                unsigned int d = wa[j] ^ wq[j];
                const int rem = ln - j * 4;
                if (rem < 4) d &= (1u << (8 * rem)) - 1u;
                neq = neq || (d != 0);
            }
            if (__any(neq) && lane == 0) parent[x] = -1;
        }
        __syncthreads();
        // ---- merges: beam x's copy entry and its parent's extension by x's last symbol are one dict entry
        if (tid < nb && parent[tid] >= 0) {
            const int x = tid, q = parent[x], e = q * C + last[x].last;
            const double pr = tot[e];
            if (q < x) {  // entry was created by the extension (inserted earlier), then the copy is added (:108-113)
                cNB[x] = log_add_prob(pr, cNB[x]);
                cT[x] = log_add_prob(pr, cT[x]);
                tot[e] = cT[x];
                tot[x * C + blank] = -INFINITY;
                mslot[x] = e;
            } else {      // entry was created by the copy, then the extension is added (:122-125)
                cNB[x] = log_add_prob(cNB[x], pr);
                cT[x] = log_add_prob(cT[x], pr);
                tot[x * C + blank] = cT[x];
                tot[e] = -INFINITY;
            }
            atomicAdd(&nmerge_s, 1);
        }
        __syncthreads();
        // ---- `last.sort()[0:beam]`: stable, descending by prTotal; insertion order = (r, copy first, then k ascending).
        // Top-`keep` of the nb*C slots under (value desc, insertion order asc), beam_kernel's three steps over a workgroup:
        //  1. theta0 = keep-th largest of the WT per-thread maxima (rank counting through LDS); at least `keep` candidates are >= theta0,
        //     so every member of the true top-`keep` is too.  With fewer finite maxima than `keep` theta0 is -inf and the list is every slot;
        //  2. the candidates >= theta0 are compacted into a list (order irrelevant), in LDS if it holds them, else in the workspace;
        //  3. each list entry counts the entries that beat it; rank < keep -> it IS output position `rank`.
        const int ncand = nslot - nmerge_s;
        const int keep = ncand < beam ? ncand : beam;
        auto idx_of = [&](int ord) {
            const int r = (int)(((float)ord + 0.5f) * invC), j = ord - r * C;
            return r * C + (j == 0 ? blank : (j <= blank ? j - 1 : j));
        };
        double lmax = -INFINITY;
        for (int idx = tid; idx < nslot; idx += WT) lmax = fmax(lmax, tot[idx]);
        tmax[tid] = lmax;
        __syncthreads();
        {
            int rk = 0;
#pragma unroll 8
            for (int j = 0; j < WT; j++) {
                const double sj = tmax[j];
                rk += (sj > lmax || (sj == lmax && j < tid)) ? 1 : 0;
            }
            if (rk == keep - 1) theta_s = lmax;
        }
        __syncthreads();
        const double theta0 = theta_s;
        int cnt = 0, pos = 0;
        if (lmax >= theta0) {
            for (int idx = tid; idx < nslot; idx += WT) cnt += (tot[idx] >= theta0) ? 1 : 0;
            pos = atomicAdd(&nlist, cnt);
        }
        __syncthreads();
        const int nl = nlist;
        auto select = [&](double *cl_v, int *cl_o) {
            if (cnt)
                for (int idx = tid; idx < nslot; idx += WT) {
                    const double v = tot[idx];
                    if (v >= theta0) {
                        const int r = (int)(((float)idx + 0.5f) * invC), k = idx - r * C;
                        cl_v[pos] = v; cl_o[pos] = beam_slot_order(r, k, C, blank); pos++;
                    }
                }
            __syncthreads();
            for (int e = tid; e < nl; e += WT) {
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
        };
        if (nl <= a.list_cap) select(lcl_v, lcl_o); else select(gcl_v, gcl_o);
        __syncthreads();
        // ---- materialise the new beams
        WideMeta *next = meta[cur ^ 1];
        if (tid < keep) {
            const int idx = sel_ord[tid];
            const int r = (int)(((float)idx + 0.5f) * invC), k = idx - r * C;
            const WideMeta &y = last[r];
            WideMeta m;
            if (k == blank) {
                m.prTotal = sel_v[tid]; m.prNonBlank = cNB[r]; m.prBlank = cB[r];
                m.len = y.len; m.last = y.last; m.hash = y.hash; m.phash = y.phash;
            } else {
                m.prTotal = sel_v[tid]; m.prNonBlank = sel_v[tid]; m.prBlank = LOG_ZERO;
                for (int x = 0; x < nb; x++)
                    if (mslot[x] == idx) { m.prNonBlank = cNB[x]; m.prBlank = cB[x]; }
                m.len = y.len + 1; m.last = k; m.phash = y.hash;
                m.hash = beam_hash_push(y.hash, k);
            }
            next[tid] = m;
        }
        // the new prefix rows, a wave per row: the parent's words, the new id put into the word it falls in by the lane that owns it
        for (int x = wave; x < keep; x += WW) {
            const int idx = sel_ord[x];
            const int r = (int)(((float)idx + 0.5f) * invC), k = idx - r * C;
            const int ln = last[r].len;
            const unsigned int *src = reinterpret_cast<const unsigned int *>(pcur + (size_t)r * Tcap);
            unsigned int *dst = reinterpret_cast<unsigned int *>(pnext + (size_t)x * Tcap);
            const bool ext = k != blank;
            const int nw = ext ? (ln >> 2) + 1 : (ln + 3) >> 2;                 // (ln + 1 <= T < Tcap, Tcap % 4 == 0: whole words inside the row)
            for (int j = lane; j < nw; j += 64) {
                unsigned int w = j * 4 < ln ? src[j] : 0u;
                if (ext && j == (ln >> 2)) {
                    const int sh = 8 * (ln & 3);
                    w = (w & ((1u << sh) - 1u)) | ((unsigned int)k << sh);
                }
                dst[j] = w;
            }
        }
        __syncthreads();
        cur ^= 1;
        nb = keep;
        e0 = e1;
        e1 = e2;
    }
    __syncthreads();
    // ---- final, N best (beam_kernel<true>'s ending): EOS LM term and length normalisation per entry (thread r = entry r of `BHat`), the
    // first failing entry in entry order decides the status, then the reference's second sort() (:29-33,148) as a rank count through LDS:
    // descending, equal scores keep their entry order.  sel_v / sel_ord are dead after the frame loop.
    const WideMeta *last = meta[cur];
    const bool act = tid < nb && !err;
    double s = -INFINITY;
    if (act) {
        const WideMeta &y = last[tid];
        int e = 0;
        if (y.len == 0) e = MDD_BEAM_INDEX_ERROR;                  // y[-1] on the empty tuple (:135)
        else {
            const double v = lmp[y.last * C1 + C];
            if (v != v) e = MDD_BEAM_KEY_ERROR;
            else s = beam_final_score(y.prTotal, v, alpha, y.len);
        }
        if (e) atomicMin(&endkey, tid * 4 + e);
    }
    if (tid < WB) { sel_v[tid] = s; sel_ord[tid] = -1; }           // entries >= nb: -inf
    __syncthreads();
    if (endkey != INT_MAX) err = endkey & 3;
    if (tid < nb) {
        int rank = 0;
        for (int j = 0; j < nb; j++) {
            const double sj = sel_v[j];
            rank += (sj > s || (sj == s && j < tid)) ? 1 : 0;
        }
        if (!err) sel_ord[rank] = tid;                              // a permutation of 0..nb-1
    }
    __syncthreads();
    const unsigned char *rows = pref + (size_t)cur * beam * Tcap;
    for (int x = wave; x < a.nbest; x += WW) {
        const int r = (err || x >= nb) ? -1 : sel_ord[x];
        const size_t o = (size_t)x * B + b;
        int ln = 0;
        if (r >= 0) {
            ln = last[r].len;
            const unsigned char *src = rows + (size_t)r * Tcap;
            for (int j = lane; j < ln; j += 64) a.ids[o * T + j] = src[j];
        }
        if (lane == 0) { a.nids[o] = ln; a.score[o] = r >= 0 ? sel_v[r] : __builtin_nan(""); }
    }
    if (tid == 0) a.status[b] = err;
}

int init_beam_wide_attributes() {
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)beam_wide_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBeamWideLdsBudget));
    MDD_HIP_CHECK(hipFuncSetAttribute((const void *)beam_wide_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBeamWideLdsBudget));
    return MDD_OK;
}

void launch_beam_wide(const BeamCall &c, const BeamWidePlan &p, unsigned char *ws) {
    BeamWideArgs a;
    a.lpw = reinterpret_cast<const double *>(ws); a.flags = ws + p.off_flags; a.utt = ws + p.off_utt;
    a.utt_bytes = p.utt; a.u_pref = p.u_pref; a.u_tot = p.u_tot; a.u_clv = p.u_clv; a.u_clo = p.u_clo;
    a.T = c.T; a.B = c.B; a.C = c.C; a.len = c.len; a.beam = c.beam; a.blank = c.blank; a.lm = c.lm; a.alpha = c.alpha; a.nbest = c.nbest;
    a.ids = c.ids; a.nids = c.nids; a.status = c.status; a.score = c.score;
    a.Tcap = p.Tcap; a.list_cap = (int)p.list_cap;
    if (p.tot_in_lds) hipLaunchKernelGGL(beam_wide_kernel<true>, dim3(c.B), dim3(WT), p.smem, c.st, a);
    else hipLaunchKernelGGL(beam_wide_kernel<false>, dim3(c.B), dim3(WT), p.smem, c.st, a);
}

}  // namespace mdd
