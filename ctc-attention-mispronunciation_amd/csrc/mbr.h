// The bit-vector edit distance of mdd_nbest_mbr (mbr.hip), host and device: one function, so that the recurrence the kernel runs is the
// one a host program can check against the plain DP (tests/test_mbr_reference.py builds it with the host compiler).
//
// Unit-cost Levenshtein distance by Myers' bit-parallel recurrence in Hyyro's block form (G. Myers, J. ACM 46(3), 1999; H. Hyyro, Nordic J.
// Computing 10, 2003): bit i of word k of Pv / Mv says that D[64 k + i + 1][j] - D[64 k + i][j] is +1 / -1 in column j of the DP matrix of
// pattern against text.  One text symbol advances a word in about 17 integer operations; the horizontal delta at a word's top bit is
// the carry into the next word, and at the pattern's last row it is the change of the distance.  The column above row 0 is D[0][j] = j:
// the carry into word 0 is always +1 (the global distance, not the search variant).
#pragma once
#include <stdint.h>

#include "plan.h"

#if defined(__HIPCC__)
#define MDD_MBR_UNROLL _Pragma("unroll")      // the word loops must unroll: Pv / Mv are registers only under constant indices
#else
#define MDD_MBR_UNROLL
#endif

namespace mdd {

// d(pattern, text) for 1 <= plen <= 64 NW and tlen >= 0.
//   peq   [C][NW] words: bit i of peq[c * NW + k] is set where pattern[64 k + i] == c, and clear at and past plen
//   text  the packed row of plan.h: word jq of the row is text[jq * stride], ids 4 jq .. 4 jq + 3 in its bytes, low byte first
// Words past the pattern's last are not touched; bits past its last row in that word hold values nothing reads (a carry only moves up).
template <int NW>
MDD_PLAN_HD inline int mbr_distance(const unsigned long long *peq, const uint32_t *text, int stride, int plen, int tlen) {
    typedef unsigned long long u64;
    u64 Pv[NW], Mv[NW];
    MDD_MBR_UNROLL
    for (int k = 0; k < NW; k++) { Pv[k] = ~0ull; Mv[k] = 0; }
    const int lastw = (plen - 1) >> 6;
    const u64 lastbit = 1ull << ((plen - 1) & 63);
    int score = plen;
    for (int j0 = 0; j0 < tlen; j0 += 4) {
        uint32_t w = text[(size_t)(j0 >> 2) * stride];
        const int n4 = tlen - j0 < 4 ? tlen - j0 : 4;
        for (int i = 0; i < n4; i++, w >>= 8) {
            const u64 *e = peq + (size_t)(w & 255u) * NW;
            int hin = 1;
            MDD_MBR_UNROLL
            for (int k = 0; k < NW; k++) {
                if (k <= lastw) {
                    u64 Eq = e[k];
                    const u64 pv = Pv[k], mv = Mv[k];
                    const u64 Xv = Eq | mv;
                    if (hin < 0) Eq |= 1;
                    const u64 Xh = (((Eq & pv) + pv) ^ pv) | Eq;
                    u64 Ph = mv | ~(Xh | pv);
                    u64 Mh = pv & Xh;
                    const u64 top = k == lastw ? lastbit : 1ull << 63;
                    const int hout = (Ph & top) ? 1 : (Mh & top) ? -1 : 0;
                    Ph <<= 1;
                    Mh <<= 1;
                    if (hin < 0) Mh |= 1;
                    if (hin > 0) Ph |= 1;
                    Pv[k] = Mh | ~(Xv | Ph);
                    Mv[k] = Ph & Xv;
                    hin = hout;
                }
            }
            score += hin;
        }
    }
    return score;
}

}  // namespace mdd
