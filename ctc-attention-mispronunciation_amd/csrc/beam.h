// What the two search kernels of the beam entries share (beam_generic.hip: beam_kernel, any shape; beam_fast.hip: beam_fast_kernel, one wave
// per utterance): the reference's constants and log-sum, the small device pieces both write the same way, and the host's call shape with
// the launchers beam.hip calls.  The LDS formulas and the route are in plan.h (beam_plan).
#pragma once
#include <type_traits>

#include "ctc_host.h"

namespace mdd {

#define LOG_ZERO (-99999999.0)  // AA/utils/BeamSearch.py:6

__device__ __forceinline__ double log_add_prob(double lx, double ly) {  // BeamSearch.py:43-50
    // branch-free (every lane evaluates the sum, the early returns are selects): the ~150 fp64 instructions can then be
    // scheduled among the neighbouring loads instead of sitting behind their own exec-mask branches
    const bool swap = (ly - lx) > 0.0;
    const double hi = swap ? ly : lx, lo = swap ? lx : ly;
    const double sum = hi + log(1 + exp(lo - hi));
    return lx <= LOG_ZERO ? ly : (ly <= LOG_ZERO ? lx : sum);
}

constexpr int MAXBEAM = kBeamMax;
constexpr int FB = kBeamFastMax;   // max beams on the fast path

// The last argument of beam_fast_kernel: the count `nbest` for the N-best ending (which takes no stamps), the stamp buffer for the winner-only
// one (mdd_diag_beam_stamps's DBG instantiation writes it; mdd_beam passes NULL), so the winner-only instantiations keep the argument block
// they always had.
template <bool NBEST> using BeamTail = typename std::conditional<NBEST, int, long long *>::type;

// The final score of a hypothesis (BeamSearch.py:130-148): the EOS LM term, then the length normalisation.
__device__ __forceinline__ double beam_final_score(double total, double eos, double alpha, int len) {
    double pr = log_add_prob(LOG_ZERO, total + eos * alpha);
    pr = pr * (1.0 / (double)(len ? len : 1));
    return pr;
}
// Rolling hash of a prefix: the empty prefix, and a prefix extended by id k.
constexpr unsigned long long BEAM_HASH_EMPTY = 0x243F6A8885A308D3ull, BEAM_HASH_MUL = 0x9E3779B97F4A7C15ull;
__device__ __forceinline__ unsigned long long beam_hash_push(unsigned long long h, int k) { return h * BEAM_HASH_MUL + (unsigned long long)(k + 1); }
// Insertion order of slot (r, k) in the reference's dict: beam r's copy entry first, then its extensions with k ascending.
__device__ __forceinline__ int beam_slot_order(int r, int k, int C, int blank) { return r * C + (k == blank ? 0 : (k < blank ? k + 1 : k)); }

// One call of a beam entry, as the entry received it.  who: the entry's name, which starts every message.  nbest_entry: mdd_beam_nbest
// (outputs hypothesis-major, score required, 1 <= nbest <= beam); else the winner alone, score optional, nbest 0.  want_stamps:
// mdd_diag_beam_stamps, whose [B,12] buffer is `stamps`; NULL for every other entry.
struct BeamCall {
    const char *who;
    bool nbest_entry, want_stamps;
    const float *logp; int T, B, C; const int32_t *len; int beam, blank; const double *lm; double alpha; int nbest;
    int32_t *ids, *nids, *status; double *score;
    long long *stamps;
    hipStream_t st;
};

// beam.hip -> beam_generic.hip, beam_fast.hip (hidden: the exported symbols stay as they were).  A launcher enqueues the search the plan chose
// on the pre-pass's outputs (lpw, flags) and leaves the launch check to its caller; an initialiser sets the LDS budget of every
// instantiation of its kernel.
__attribute__((visibility("hidden"))) void launch_beam_generic(const BeamCall &c, const BeamPlan &p, const double *lpw, const unsigned char *flags);
__attribute__((visibility("hidden"))) void launch_beam_fast(const BeamCall &c, const BeamPlan &p, const double *lpw, const unsigned char *flags);
__attribute__((visibility("hidden"))) int init_beam_generic_attributes();
__attribute__((visibility("hidden"))) int init_beam_fast_attributes();
// beam.hip -> beam_wide.hip (mdd_beam_wide): the wide kernel on the workspace the plan laid out, whose head the pre-pass has filled
__attribute__((visibility("hidden"))) void launch_beam_wide(const BeamCall &c, const BeamWidePlan &p, unsigned char *ws);
__attribute__((visibility("hidden"))) int init_beam_wide_attributes();

}  // namespace mdd
