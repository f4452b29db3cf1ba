// CTC prefix beam search, the single-wave kernel (the reference, the pre-pass and the host path: beam.hip; the generic kernel, whose
// comments explain the algorithm's steps: beam_generic.hip).
#include "beam.h"

namespace mdd {

// ---- pass 2, fast path (beam <= 16, C <= 64): same algorithm, restructured for a single wave's latency.
// A lone wave pays ~100 cycles for every dependent LDS round trip, so the work is arranged in unrolled phases whose
// loads are all independent: slots are dealt to lanes round-robin (slot = lane + 64 i, coordinates precomputed once),
// the beam state is a structure of arrays, candidate operands are gathered before anything is stored, the top-`beam`
// selection reads each lane's slots into registers once and then uses wave ballots / v_readlane only:
//   lane maxima -> rank by v_readlane broadcast -> theta0 (keep-th largest lane maximum; because slots are dealt
//   round-robin the true winners sit in different lanes and theta0 is tight) -> ballot compaction of the ~10-20
//   candidates >= theta0 -> rank counting among those (rank < keep IS the output position).
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// Workgroup shape: W = blockDim.x / 64 independent waves, one utterance each, sharing only the LM table.  A beam wave
// holds ~210 VGPRs, so a CU that hosts one cannot take a workgroup of the forward's GEMM (2 x 256 VGPRs per SIMD) or
// persistent BiLSTM (414): dealt one wave per CU the search would fence the whole chip off from the next batch's
// forward for its entire duration.  Packed W = 4 to a CU (one per SIMD, each with the full 512-VGPR budget so that a
// phase's loads can all be in flight) it occupies B / 4 CUs and the forward keeps the rest.  Waves never meet at a workgroup barrier after the LM load
// (utterance lengths differ); inside a wave, LDS operations complete in order, so a wave-scope fence is the only
// synchronisation between the phases.
#define BEAM_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// LDS bytes of one wave's private state and of the shared LM table: beam_fast_wave_bytes, beam_fast_lm_bytes (plan.h, shared with the plan)

// Coding rules of this kernel (a lone wave pays ~120 cycles per dependent LDS round trip and ~4 cycles per VALU
// instruction, and the compiler turns every conditional load into a branch with its own wait):
//   * loads are unconditional, from clamped (always valid) addresses, gathered at the top of a phase; conditions are
//     applied to registers afterwards; per-beam arrays of FB entries are read whole with 16-byte loads;
//   * everything wave-uniform (frame counters, beam count, keep, list lengths) is forced into SGPRs with
//     v_readfirstlane so that the control flow stays scalar;
//   * per-beam values (copy-path scores, parent, merge slot) stay in the registers of lane == beam and move between
//     lanes with v_readlane / ballots rather than through LDS.
// NBEST selects the ending, as in beam_kernel.
template <int NS, bool DBG, bool NBEST>
__global__ __launch_bounds__(256) void beam_fast_kernel(const double *__restrict__ lpw, const unsigned char *__restrict__ flags,
                                                       int T, int B, int C, const int32_t *__restrict__ len, int beam, int blank,
                                                       const double *__restrict__ lm, double alpha, int32_t *__restrict__ ids,
                                                       int32_t *__restrict__ nids, int32_t *__restrict__ status,
                                                       double *__restrict__ score, int Tcap, BeamTail<NBEST> tail) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    const int C1 = C + 1;
    long long *__restrict__ dbg = nullptr;
    int nbest = 0;
    if constexpr (NBEST) nbest = tail; else dbg = tail;
    (void)nbest; (void)dbg;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    double *lmt = reinterpret_cast<double *>(sm);                      // [C1*C1], shared by the waves
    unsigned char *mine = sm + beam_fast_lm_bytes(C) + (size_t)wave * ((beam_fast_wave_bytes(NS, beam, Tcap) + 15) & ~(size_t)15);
    double *tot = reinterpret_cast<double *>(mine);                    // [NS*64]
    double *cl_v = tot + NS * 64;                                      // [NS*64] compacted candidates: value,
    double *lp = cl_v + NS * 64;                                       // [64]
    double (*m_T)[FB] = reinterpret_cast<double (*)[FB]>(lp + 64);     // [2][FB] beam state, double-buffered
    double (*m_NB)[FB] = m_T + 2, (*m_B)[FB] = m_NB + 2;
    double *cNB = reinterpret_cast<double *>(m_B + 2), *cB = cNB + FB, *cT = cB + FB, *sel_v = cT + FB;
    unsigned long long (*m_hash)[FB] = reinterpret_cast<unsigned long long (*)[FB]>(sel_v + FB), (*m_phash)[FB] = m_hash + 2;
    int *cl_o = reinterpret_cast<int *>(m_phash + 2);                  //   insertion order,
    int *cl_x = cl_o + NS * 64;                                        //   slot index
    int (*m_len)[FB] = reinterpret_cast<int (*)[FB]>(cl_x + NS * 64), (*m_last)[FB] = m_len + 2;
    int *mslot = reinterpret_cast<int *>(m_last + 2), *sel_x = mslot + FB;
    unsigned char *fl = reinterpret_cast<unsigned char *>(sel_x + FB);
    unsigned char *pref = fl + Tcap;

    for (int i = threadIdx.x; i < C1 * C1; i += blockDim.x) lmt[i] = lm[i];
    __syncthreads();                                                   // the only workgroup barrier
    const int b = blockIdx.x * (blockDim.x >> 6) + wave;
    if (b >= B) return;
    int cur = 0, nb = 1, err = 0;
    long long ph[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tstamp = 0;   // DBG (mdd_diag_beam_stamps): cycles per phase
#define FSTAMP(i) do { if (DBG) { long long now_ = __builtin_readcyclecounter(); ph[i] += now_ - tstamp; tstamp = now_; } } while (0)
    if (lane < FB) {   // beam 0 = the empty prefix; the other entries only need to be valid numbers
        m_T[0][lane] = 0.0; m_B[0][lane] = 0.0; m_NB[0][lane] = LOG_ZERO; m_len[0][lane] = lane == 0 ? 0 : -2; m_last[0][lane] = -1;
        m_hash[0][lane] = BEAM_HASH_EMPTY; m_phash[0][lane] = 0;
        m_T[1][lane] = 0.0; m_B[1][lane] = 0.0; m_NB[1][lane] = LOG_ZERO; m_len[1][lane] = 0; m_last[1][lane] = -1;
        m_hash[1][lane] = 0; m_phash[1][lane] = 0;
        mslot[lane] = -1; sel_x[lane] = 0; sel_v[lane] = 0.0; cNB[lane] = 0.0; cB[lane] = 0.0;
    }
    int tl = __builtin_amdgcn_readfirstlane(len[b]);
    tl = tl < 0 ? 0 : (tl > T ? T : tl);
    for (int i = lane; i < tl; i += 64) fl[i] = flags[(size_t)i * B + b];
    // slot coordinates of this lane (constant over the whole utterance): slot = lane + 64 i = r*C + k
    // (kept as data, not as hoisted lane masks: a dozen loop-invariant 64-bit masks cost more SGPRs than the wave has)
    int sr[NS], sk[NS], sx[NS];                                        // sx: the slot index, or a huge one for copy slots (k == blank)
#pragma unroll
    for (int i = 0; i < NS; i++) {
        const int idx = lane + 64 * i;
        sr[i] = idx / C; sk[i] = idx - sr[i] * C;
        sx[i] = sk[i] == blank ? 0x7fffffff : idx;
    }
    const float invC = 1.0f / (float)C;
    const int nw = Tcap >> 2;                                          // words per prefix row
    const int li = lane & (FB - 1);                                    // the beam this lane speaks for (lanes >= FB: a valid alias)
    BEAM_WAVE_SYNC();

    int t = 0;
    while (t < tl && !(__builtin_amdgcn_readfirstlane(fl[t]) & 1)) t++;
    double pre = (t < tl && lane < C) ? lpw[((size_t)t * B + b) * C + lane] : 0.0;
    if (DBG) tstamp = __builtin_readcyclecounter();
    while (t < tl) {
        const bool rep_ok = (__builtin_amdgcn_readfirstlane(fl[t]) & 2) != 0;
        if (lane < C) lp[lane] = pre;
        int tn = t + 1;
        while (tn < tl && !(__builtin_amdgcn_readfirstlane(fl[tn]) & 1)) tn++;
        pre = (tn < tl && lane < C) ? lpw[((size_t)tn * B + b) * C + lane] : 0.0;
        BEAM_WAVE_SYNC();
        const unsigned int *srcw = reinterpret_cast<const unsigned int *>(pref + (size_t)cur * FB * Tcap);
        unsigned char *pnext = pref + (size_t)(cur ^ 1) * FB * Tcap;
        const int nslot = nb * C;

        FSTAMP(0);
        // ---- candidate scores (BeamSearch.py:53-69): gather every operand, then store.  errp = (order << 2 | kind) of
        // the first failure in the reference's execution order (kind 1: LM KeyError, 2: log(0) ValueError)
        int errp = 0x7fffffff;
        double val[NS];
#pragma unroll
        for (int i = 0; i < NS; i++) {
            const int r = min(sr[i], nb - 1), k = sk[i];
            const int ylen = m_len[cur][r], ylast = m_last[cur][r];
            const double yB = m_B[cur][r], yT = m_T[cur][r];
            const double lmv = lmt[(ylen ? ylast : C) * C1 + k];   // consulted even when alpha == 0 (BeamSearch.py:57-60)
            const double lk = lp[k];
            const bool live = sx[i] < nslot;                             // an extension slot of a beam that exists
            const int kind = (lmv != lmv) ? 1 : ((lk == -INFINITY) ? 2 : 0);
            const int e = (live && kind) ? (((sr[i] * C1 + 1 + k) << 2) | kind) : 0x7fffffff;
            errp = min(errp, e);
            const double base = (ylen && ylast == k && rep_ok) ? yB : yT;   // :63-66
            val[i] = live ? lk + lmv * alpha + base : -INFINITY;
        }
#pragma unroll
        for (int i = 0; i < NS; i++) tot[lane + 64 * i] = val[i];        // copy slots (k == blank) are overwritten just below
        FSTAMP(1);
        // ---- copy path of beam `li` (:101-113), and the beam (if any) that holds its prefix minus the last id
        const int ylen = m_len[cur][li], ylast = m_last[cur][li];
        double pnb, pb, tc;
        int par = -1;
        {
            const double lpb = lp[blank], lpl = lp[max(ylast, 0)];
            const double mNB = m_NB[cur][li], mT = m_T[cur][li];
            const unsigned long long myph = m_phash[cur][li];
            i32x4 L4[FB / 4];
            u64x2 H2[FB / 2];
#pragma unroll
            for (int q = 0; q < FB / 4; q++) L4[q] = reinterpret_cast<const i32x4 *>(m_len[cur])[q];
#pragma unroll
            for (int q = 0; q < FB / 2; q++) H2[q] = reinterpret_cast<const u64x2 *>(m_hash[cur])[q];
            pnb = ylen > 0 ? mNB + lpl : LOG_ZERO;
            pb = mT + lpb;
            const bool bad = lpb == -INFINITY || (ylen > 0 && lpl == -INFINITY);
            if (lane < nb && bad) errp = min(errp, ((lane * C1) << 2) | 2);
            tc = log_add_prob(pb, pnb);
#pragma unroll
            for (int q = FB - 1; q >= 0; q--) {                          // the lowest matching q wins
                const bool hit = L4[q >> 2][q & 3] == ylen - 1 && H2[q >> 1][q & 1] == myph;   // entries >= nb hold length -2
                par = hit ? q : par;
            }
            par = (lane < nb && ylen > 0) ? par : -1;
            if (lane < nb) tot[lane * C + blank] = tc;
        }
        FSTAMP(2);
        // verify the content of every hash match with the whole wave (never merge on a hash collision): all pairs at once
        {
            const unsigned int pm = (unsigned int)__ballot(par >= 0);    // beams with a parent candidate (bits < FB)
            if (pm) {
                unsigned int neq = 0;
                for (int j0 = 0; j0 < nw; j0 += 64) {
                    const int j = min(j0 + lane, nw - 1);
                    unsigned int wa[FB], wq[FB];
#pragma unroll
                    for (int a = 0; a < FB; a++) {
                        const int qa = max(__builtin_amdgcn_readlane(par, a), 0);
                        wa[a] = srcw[a * nw + j];
                        wq[a] = srcw[qa * nw + j];
                    }
#pragma unroll
                    for (int a = 0; a < FB; a++) {
                        const int rem = __builtin_amdgcn_readlane(ylen, a) - 1 - 4 * j;      // bytes of the parent's prefix from word j on
                        const unsigned int m = rem >= 4 ? 0xffffffffu : (rem <= 0 ? 0u : ((1u << (8 * rem)) - 1u));
                        neq |= (((wa[a] ^ wq[a]) & m) != 0 ? 1u : 0u) << a;
                    }
                }
                unsigned int bad = 0;
#pragma unroll
                for (int a = 0; a < FB; a++) bad |= (__any((neq >> a) & 1) ? 1u : 0u) << a;
                if ((bad >> li) & 1) par = -1;
            }
        }
        FSTAMP(3);
        if (__any(errp != 0x7fffffff)) {   // first error in the reference's execution order wins
            int eo = errp;
            for (int o = 32; o > 0; o >>= 1) eo = min(eo, __shfl_xor(eo, o));
            err = (eo & 3) == 1 ? MDD_BEAM_KEY_ERROR : MDD_BEAM_VALUE_ERROR;
            break;
        }
        BEAM_WAVE_SYNC();
        FSTAMP(4);
        // ---- merges (see beam_kernel): a beam whose prefix is also reachable as parent + last id takes both paths
        int ms = -1;
        const bool merging = par >= 0;
        const int nmerge = __popcll(__ballot(merging));
        if (nmerge) {
            const int q = max(par, 0), e = q * C + max(ylast, 0);
            const double pr = tot[e];
            const bool fwd = q < lane;                                    // the extension was inserted before the copy
            const double nNB = log_add_prob(fwd ? pr : pnb, fwd ? pnb : pr);
            const double nT = log_add_prob(fwd ? pr : tc, fwd ? tc : pr);
            if (merging) {
                pnb = nNB; tc = nT;
                tot[fwd ? e : lane * C + blank] = nT;
                tot[fwd ? lane * C + blank : e] = -INFINITY;
                ms = fwd ? e : -1;
            }
        }
        if (lane < FB) { cNB[lane] = pnb; cB[lane] = pb; mslot[lane] = lane < nb ? ms : -1; }
        BEAM_WAVE_SYNC();
        FSTAMP(5);
        // ---- top-`keep` selection
        const int ncand = nslot - nmerge;
        const int keep = ncand < beam ? ncand : beam;
        double tv[NS];
#pragma unroll
        for (int i = 0; i < NS; i++) tv[i] = tot[lane + 64 * i];     // slots >= nslot hold -inf
        double lmax = tv[0];
#pragma unroll
        for (int i = 1; i < NS; i++) lmax = fmax(lmax, tv[i]);
        // rank of the lane maximum = lane maxima strictly above it, counted against LDS broadcasts (two per read);
        // theta0 = the smallest lane maximum of rank < keep: at least `keep` slots are >= theta0
        cl_v[lane] = lmax;
        BEAM_WAVE_SYNC();
        int rk = 0;
#pragma unroll
        for (int h = 0; h < 2; h++) {   // two rounds of 16 reads, all of a round in flight before the first compare
            f64x2 sj[16];
#pragma unroll
            for (int j = 0; j < 16; j++) sj[j] = reinterpret_cast<const f64x2 *>(cl_v)[16 * h + j];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 16; j++) rk += (sj[j].x > lmax ? 1 : 0) + (sj[j].y > lmax ? 1 : 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        unsigned long long mk = 0;
        for (int r = keep - 1; r >= 0 && mk == 0; r--) mk = __ballot(rk == r);
        const int srcl = __ffsll((long long)mk) - 1;
        const double theta0 = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(lmax), srcl),
                                               __builtin_amdgcn_readlane(__double2loint(lmax), srcl));
        BEAM_WAVE_SYNC();                                                // cl_v is rewritten by the compaction below
        FSTAMP(6);
        int nl = 0;
        const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
        for (int i = 0; i < NS; i++) {
            const bool pred = tv[i] >= theta0;                           // theta0 is finite, slots >= nslot hold -inf
            const unsigned long long msk = __ballot(pred);
            if (msk) {
                if (pred) {
                    const int pos = nl + __popcll(msk & lt), k = sk[i];
                    cl_v[pos] = tv[i]; cl_x[pos] = lane + 64 * i;
                    cl_o[pos] = beam_slot_order(sr[i], k, C, blank);                      // insertion order of the slot
                }
                nl += __popcll(msk);
            }
        }
        BEAM_WAVE_SYNC();
        FSTAMP(7);
        if (nl <= 64) {   // the usual case: one candidate per lane, ranked against v_readlane broadcasts
            const bool has = lane < nl;
            const double v_ld = cl_v[lane];                               // unconditional: three loads in flight, not three branches
            const int o_ld = cl_o[lane], xs = cl_x[lane];
            const double v = has ? v_ld : -INFINITY;
            const int o = has ? o_ld : 0x7fffffff;
            const int vlo = __double2loint(v), vhi = __double2hiint(v);
            int rank = 0;
            for (int f = 0; f < nl; f++) {
                const double vf = __hiloint2double(__builtin_amdgcn_readlane(vhi, f), __builtin_amdgcn_readlane(vlo, f));
                const int of = __builtin_amdgcn_readlane(o, f);
                rank += (vf > v || (vf == v && of < o)) ? 1 : 0;
            }
            if (has && rank < keep) { sel_v[rank] = v; sel_x[rank] = xs; }
        } else
        for (int e = lane; e < nl; e += 64) {
            const double v = cl_v[e];
            const int o = cl_o[e];
            int rank = 0;
#pragma unroll 4
            for (int f = 0; f < nl; f++) {
                const double vf = cl_v[f];
                const int of = cl_o[f];
                rank += (vf > v || (vf == v && of < o)) ? 1 : 0;
            }
            if (rank < keep) { sel_v[rank] = v; sel_x[rank] = cl_x[e]; }
        }
        BEAM_WAVE_SYNC();
        FSTAMP(8);
        if (DBG) ph[11] += nl;
        // ---- materialise new beam `li` (lanes >= keep compute on stale but valid entries and store nothing)
        const int nxt = cur ^ 1;
        int r_new, app_k, app_at;                                         // parent row; id appended (-1: none) and where
        {
            const int idx = sel_x[li];
            const double v = sel_v[li];
            i32x4 M4[FB / 4];
#pragma unroll
            for (int a = 0; a < FB / 4; a++) M4[a] = reinterpret_cast<const i32x4 *>(mslot)[a];
            const int r = min((int)(((float)idx + 0.5f) * invC), FB - 1), k = idx - r * C;
            const double cNBr = cNB[r], cBr = cB[r];
            const int len_r = m_len[cur][r], last_r = m_last[cur][r];
            const unsigned long long hash_r = m_hash[cur][r], phash_r = m_phash[cur][r];
            int fa = -1;                                                  // the beam merged into this extension, if any
#pragma unroll
            for (int a = 0; a < FB; a++) fa = M4[a >> 2][a & 3] == idx ? a : fa;   // entries >= nb hold -1
            const double cNBa = cNB[max(fa, 0)], cBa = cB[max(fa, 0)];
            const bool isb = k == blank;
            r_new = r; app_k = isb ? -1 : k; app_at = len_r;
            if (lane < FB) {   // entries keep..FB-1 get length -2: no prefix is their child (parent search above)
                const bool on = lane < keep;
                m_T[nxt][lane] = v;
                m_NB[nxt][lane] = isb ? cNBr : (fa >= 0 ? cNBa : v);
                m_B[nxt][lane] = isb ? cBr : (fa >= 0 ? cBa : LOG_ZERO);
                m_len[nxt][lane] = on ? (isb ? len_r : len_r + 1) : -2;
                m_last[nxt][lane] = on ? (isb ? last_r : k) : -1;
                m_hash[nxt][lane] = isb ? hash_r : beam_hash_push(hash_r, k);
                m_phash[nxt][lane] = isb ? phash_r : hash_r;
            }
        }
        FSTAMP(9);
        {   // prefixes: every new beam copies its parent's whole row (bytes past a prefix's length are never read),
            // one word per lane and row, all rows in flight together; the appended id goes in afterwards
            // (rows keep..FB-1 receive a copy of some valid row: harmless, and it keeps every load and store unconditional)
            int rr[FB];
#pragma unroll
            for (int i = 0; i < FB; i++) rr[i] = __builtin_amdgcn_readlane(r_new, i);
            unsigned int *dstw = reinterpret_cast<unsigned int *>(pnext);
            for (int j = lane; j < nw; j += 64) {
                unsigned int w[FB];
#pragma unroll
                for (int i = 0; i < FB; i++) w[i] = srcw[rr[i] * nw + j];
#pragma unroll
                for (int i = 0; i < FB; i++) dstw[i * nw + j] = w[i];
            }
            BEAM_WAVE_SYNC();
            if (lane < keep && app_k >= 0) pnext[(size_t)lane * Tcap + app_at] = (unsigned char)app_k;
        }
        BEAM_WAVE_SYNC();
        cur = nxt;
        nb = keep;
        t = tn;
        FSTAMP(10);
    }
    BEAM_WAVE_SYNC();
    if constexpr (NBEST) {
        // final, N best (see beam_kernel): lane r speaks for entry r, its score stays in the lane; status and ranks come from
        // ballots and v_readlane broadcasts, then the lanes of the wave stride each ranked prefix row, bytes to int32
        err = __builtin_amdgcn_readfirstlane(err);
        const int ylen = m_len[cur][li], ylast = m_last[cur][li];
        const double mT = m_T[cur][li];
        const double v = lmt[max(ylast, 0) * C1 + C];
        const bool act = lane < nb && !err;
        const int e = !act ? 0 : (ylen == 0 ? MDD_BEAM_INDEX_ERROR : (v != v ? MDD_BEAM_KEY_ERROR : 0));   // y[-1] on the empty tuple (:135)
        const double pr = beam_final_score(mT, v, alpha, ylen);
        const double s = (act && !e) ? pr : -INFINITY;
        const unsigned long long em = __ballot(e != 0);
        if (em) err = __builtin_amdgcn_readlane(e, __ffsll((long long)em) - 1);   // the first failing entry in entry order
        const int slo = __double2loint(s), shi = __double2hiint(s);
        int rank = 0;
        for (int j = 0; j < nb; j++) {
            const double sj = __hiloint2double(__builtin_amdgcn_readlane(shi, j), __builtin_amdgcn_readlane(slo, j));
            rank += (sj > s || (sj == s && j < lane)) ? 1 : 0;
        }
        const unsigned char *rows = pref + (size_t)cur * FB * Tcap;
        for (int n = 0; n < nbest; n++) {
            const unsigned long long hm = err ? 0ull : __ballot(lane < nb && rank == n);
            const size_t o = (size_t)n * B + b;
            int ln = 0;
            double sc = __builtin_nan("");
            if (hm) {
                const int r = __ffsll((long long)hm) - 1;
                ln = __builtin_amdgcn_readlane(ylen, r);
                sc = __hiloint2double(__builtin_amdgcn_readlane(shi, r), __builtin_amdgcn_readlane(slo, r));
                const unsigned char *src = rows + (size_t)r * Tcap;
                for (int j = lane; j < ln; j += 64) ids[o * T + j] = src[j];
            }
            if (lane == 0) { nids[o] = ln; score[o] = sc; }
        }
        if (lane == 0) status[b] = err;
    } else
    if (lane == 0) {   // final: EOS LM term, length normalisation, first maximum (:130-148)
        int best = -1;
        double bestv = 0.0;
        for (int r = 0; r < nb && !err; r++) {
            const int ylen = m_len[cur][r];
            if (ylen == 0) { err = MDD_BEAM_INDEX_ERROR; break; }
            const double v = lmt[m_last[cur][r] * C1 + C];
            if (v != v) { err = MDD_BEAM_KEY_ERROR; break; }
            const double pr = beam_final_score(m_T[cur][r], v, alpha, ylen);
            if (best < 0 || pr > bestv) { best = r; bestv = pr; }
        }
        status[b] = err;
        int n = 0;
        if (!err && best >= 0) {
            n = m_len[cur][best];
            const unsigned char *src = pref + (size_t)cur * FB * Tcap + (size_t)best * Tcap;
            for (int j = 0; j < n; j++) ids[(size_t)b * T + j] = src[j];
        }
        nids[b] = n;
        if (score) score[b] = err ? __builtin_nan("") : bestv;
        if (DBG) for (int i = 0; i < 12; i++) dbg[b * 12 + i] = ph[i];
    }
#undef FSTAMP
}

// The six instantiations, named once: f(NS, DBG, NBEST as integral constants) for the slots per lane the plan chose (8 or 16) and the
// ending -- the winner alone, the winner with phase stamps, or the N best (which take no stamps).  false: no such instantiation.
template <int NS, class F> static bool with_beam_fast_ending(bool dbg, bool nbest, F f) {
    using ns = std::integral_constant<int, NS>;
    if (dbg && nbest) return false;
    if (nbest) f(ns{}, std::false_type{}, std::true_type{});
    else if (dbg) f(ns{}, std::true_type{}, std::false_type{});
    else f(ns{}, std::false_type{}, std::false_type{});
    return true;
}
template <class F> static bool with_beam_fast(int ns, bool dbg, bool nbest, F f) {
    if (ns == 8) return with_beam_fast_ending<8>(dbg, nbest, f);
    if (ns == 16) return with_beam_fast_ending<16>(dbg, nbest, f);
    return false;
}

int init_beam_fast_attributes() {
    for (const int ns : {8, 16})
        for (const int ending : {0, 1, 2}) {   // winner, winner + stamps, N best
            hipError_t e = hipSuccess;
            with_beam_fast(ns, ending == 1, ending == 2, [&](auto NS, auto DBG, auto NB) {
                e = hipFuncSetAttribute((const void *)beam_fast_kernel<decltype(NS)::value, decltype(DBG)::value, decltype(NB)::value>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBeamFastLdsMax);
            });
            MDD_HIP_CHECK(e);
        }
    return MDD_OK;
}

// p.W waves (utterances) per workgroup; c.stamps selects the stamped instantiation (winner-only ending)
void launch_beam_fast(const BeamCall &c, const BeamPlan &p, const double *lpw, const unsigned char *flags) {
    const size_t fs = p.lmb + (size_t)p.W * p.pw;
    const dim3 grid((c.B + p.W - 1) / p.W), block(64 * p.W);
    with_beam_fast(p.NS, c.stamps != nullptr, p.nbest, [&](auto NS, auto DBG, auto NB) {
        BeamTail<decltype(NB)::value> tail;
        if constexpr (decltype(NB)::value) tail = c.nbest; else tail = c.stamps;
        hipLaunchKernelGGL((beam_fast_kernel<decltype(NS)::value, decltype(DBG)::value, decltype(NB)::value>), grid, block, fs, c.st, lpw, flags, c.T,
                           c.B, c.C, c.len, c.beam, c.blank, c.lm, c.alpha, c.ids, c.nids, c.status, c.score, p.Tcap, tail);
    });
}

}  // namespace mdd
