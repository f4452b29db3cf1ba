// CTC decoders on the GPU: prefix beam search (greedy: greedy.hip).  The frame pre-pass and the host path of the beam entries; the two
// search kernels are in beam_generic.hip and beam_fast.hip, what they share in beam.h, the LDS limits and the route in plan.h (beam_plan).
// mdd_beam_wide (beam <= 256, any T up to 38400) is a third kernel behind its own entry: beam_wide.hip, laid out by plan.h's beam_wide_plan.
//
// Reference: BeamDecoder.decode -> ctcBeamSearch.decode (AA/utils/ctcDecoder.py:215-226, AA/utils/BeamSearch.py:73-153).
// A serial scan over the posterior frames of one utterance; it is latency-bound, not bandwidth- or flop-bound (180 B read per frame).
#include "beam.h"

namespace mdd {

// ---- pass 1 (parallel over frames): everything about a frame that does not depend on the beam state.
//   lp[t,b,c]   = log((double)p) with p = fp32(exp(logp))   (-inf where p == 0: the reference raises ValueError
//                 when such a value is needed, BeamSearch.py:64,66,103,106)
//   flags[t,b]  bit0: frame is live, i.e. NOT (1 - p_blank < 0.1) in float32 (BeamSearch.py:93-94)
//               bit1: p_blank of the raw previous frame < 0.9 in float32 (the repeat rule, :63)
// exp() is evaluated in fp64 and rounded once, so p is the correctly rounded fp32 value the reference's
// torch.exp (ctcDecoder.py:224) produces on ~99% of inputs (<= 1 ulp otherwise).
__global__ __launch_bounds__(256) void beam_prep_kernel(const float *__restrict__ logp, int T, int B, int C, int blank,
                                                        double *__restrict__ lp, unsigned char *__restrict__ flags) {
    const size_t n = (size_t)T * B * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float p = (float)exp((double)logp[i]);
        lp[i] = p > 0.0f ? log((double)p) : -INFINITY;
        const size_t tb = i / C;
        if ((int)(i - tb * C) == blank) {
            unsigned char f = ((1.0f - p) < 0.1f) ? 0 : 1;
            const size_t t = tb / B;
            if (t > 0) {
                const float pprev = (float)exp((double)logp[i - (size_t)B * C]);
                if (pprev < 0.9f) f |= 2;
            }
            flags[tb] = f;
        }
    }
}

// The one host path of the beam entries, in the order of ctc_host.h: refuse (arguments, then the plan's LDS limits), attributes once per
// device, workspace, pre-pass, the search kernel the plan chose, launch check.  Every refusal comes before any device work.
static int beam_search(const BeamCall &c) {
    if (!c.logp || !c.len || !c.lm || !c.ids || !c.nids || !c.status || c.T <= 0 || c.B <= 0 || c.C <= 1 || c.C > 256 || c.beam < 1 ||
        c.beam > MAXBEAM || c.blank < 0 || c.blank >= c.C) {
        set_error("%s: bad argument (need 1<=beam<=64, 2<=C<=256)", c.who); return MDD_ERR_ARG;
    }
    if (c.nbest_entry && (c.nbest < 1 || c.nbest > c.beam || !c.score)) {
        set_error("%s: bad argument (need 1<=nbest<=beam and score_dev)", c.who); return MDD_ERR_ARG;
    }
    if (c.want_stamps && !c.stamps) { set_error("%s: bad argument (stamps_dev)", c.who); return MDD_ERR_ARG; }
    const BeamPlan p = beam_plan(c.T, c.B, c.C, c.beam, c.nbest_entry, read_beam_switches());
    if (p.over == BeamLimit::GenericLds) { set_error("%s: beam*C / T too large for LDS (%zu B)", c.who, p.over_bytes); return MDD_ERR_ARG; }
    if (p.over == BeamLimit::FastLds) { set_error("%s: T too long for LDS (%zu B)", c.who, p.over_bytes); return MDD_ERR_ARG; }
    if (c.want_stamps && !p.fast) { set_error("%s: the shape is not routed to the single-wave kernel, which alone writes stamps", c.who); return MDD_ERR_ARG; }
    static OncePerDevice once;
    const int arc = once_per_device(once, []() -> int {
        if (int rc = init_beam_generic_attributes()) return rc;
        return init_beam_fast_attributes();
    });
    if (arc) return arc;
    // stream-ordered scratch for the frame pre-pass: log-probabilities in fp64 + per-frame flags
    const size_t n = (size_t)c.T * c.B * c.C;
    StreamWorkspace ws;
    if (int rc = ws.acquire(nullptr, (int64_t)(n * sizeof(double) + (size_t)c.T * c.B), c.st)) return rc;
    double *lpw = ws.as<double>();
    unsigned char *flags = reinterpret_cast<unsigned char *>(lpw + n);
    int grid = (int)((n + 255) / 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(beam_prep_kernel, dim3(grid), dim3(256), 0, c.st, c.logp, c.T, c.B, c.C, c.blank, lpw, flags);
    if (p.fast) launch_beam_fast(c, p, lpw, flags); else launch_beam_generic(c, p, lpw, flags);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { set_error("beam kernel launch failed: %s", hipGetErrorString(le)); return MDD_ERR_HIP; }
    return MDD_OK;
}

}  // namespace mdd

using namespace mdd;

extern "C" int mdd_beam(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, int32_t beam,
                        int32_t blank, const double *lm_dev, double lm_alpha, int32_t *ids_dev, int32_t *nids_dev,
                        int32_t *status_dev, double *score_dev, void *stream) {
    return beam_search({"mdd_beam", false, false, logp_dev, T, B, C, len_dev, beam, blank, lm_dev, lm_alpha, 0, ids_dev, nids_dev, status_dev, score_dev,
                        nullptr, (hipStream_t)stream});
}

extern "C" int mdd_beam_nbest(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, int32_t beam,
                              int32_t blank, const double *lm_dev, double lm_alpha, int32_t nbest, int32_t *ids_dev,
                              int32_t *nids_dev, int32_t *status_dev, double *score_dev, void *stream) {
    return beam_search({"mdd_beam_nbest", true, false, logp_dev, T, B, C, len_dev, beam, blank, lm_dev, lm_alpha, nbest, ids_dev, nids_dev, status_dev,
                        score_dev, nullptr, (hipStream_t)stream});
}

// Whether mdd_beam / mdd_beam_nbest accept the shape now: their argument ranges and their plan's limits, under the switches they would read
extern "C" int32_t mdd_beam_fits(int32_t T, int32_t B, int32_t C, int32_t beam) {
    if (!beam_shape_ok(T, B, C, beam)) return 0;
    return beam_plan(T, B, C, beam, false, read_beam_switches()).over == BeamLimit::Ok ? 1 : 0;
}

// bytes of workspace mdd_beam_wide needs for these shapes (beam_wide_plan): the pre-pass's outputs and one slice per utterance
extern "C" int64_t mdd_beam_wide_workspace_bytes(int32_t T, int32_t B, int32_t C, int32_t beam) {
    if (!beam_wide_shape_ok(T, B, C, beam)) return 0;
    return (int64_t)beam_wide_plan(T, B, C, beam).bytes;
}

// The wide entry, in the order of ctc_host.h.  No switches: one kernel, chosen by nothing but the plan's LDS placement.
extern "C" int mdd_beam_wide(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, int32_t beam, int32_t blank,
                             const double *lm_dev, double lm_alpha, int32_t nbest, int32_t *ids_dev, int32_t *nids_dev,
                             int32_t *status_dev, double *score_dev, void *workspace_dev, int64_t workspace_bytes, void *stream) {
    const char *what = !logp_dev ? "logp_dev is NULL" : !len_dev ? "len_dev is NULL" : !lm_dev ? "lm_dev is NULL" : !ids_dev ? "ids_dev is NULL"
                     : !nids_dev ? "nids_dev is NULL" : !status_dev ? "status_dev is NULL" : !score_dev ? "score_dev is NULL"
                     : (T < 1 || T > kBeamWideMaxT) ? "need 1<=T<=38400" : B < 1 ? "B < 1" : (C < 2 || C > 256) ? "need 2<=C<=256"
                     : (beam < 1 || beam > kBeamWideMax) ? "need 1<=beam<=256" : (blank < 0 || blank >= C) ? "blank outside [0, C)"
                     : (nbest < 1 || nbest > beam) ? "need 1<=nbest<=beam" : nullptr;
    if (what) { set_error("mdd_beam_wide: bad argument (%s)", what); return MDD_ERR_ARG; }
    const BeamWidePlan p = beam_wide_plan(T, B, C, beam);
    if (workspace_dev && workspace_bytes < (int64_t)p.bytes)
        return refuse_workspace("mdd_beam_wide", "mdd_beam_wide_workspace_bytes", workspace_bytes, (int64_t)p.bytes);
    hipStream_t st = (hipStream_t)stream;
    static OncePerDevice once;
    if (int rc = once_per_device(once, init_beam_wide_attributes)) return rc;
    StreamWorkspace ws;
    if (int rc = ws.acquire(workspace_dev, (int64_t)p.bytes, st)) return rc;
    unsigned char *w = ws.as<unsigned char>();
    const size_t n = (size_t)T * B * C;
    int grid = (int)((n + 255) / 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(beam_prep_kernel, dim3(grid), dim3(256), 0, st, logp_dev, T, B, C, blank, reinterpret_cast<double *>(w), w + p.off_flags);
    const BeamCall c{"mdd_beam_wide", true, false, logp_dev, T, B, C, len_dev, beam, blank, lm_dev, lm_alpha, nbest, ids_dev, nids_dev, status_dev,
                     score_dev, nullptr, st};
    launch_beam_wide(c, p, w);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { set_error("mdd_beam_wide: kernel launch failed: %s", hipGetErrorString(le)); return MDD_ERR_HIP; }
    return MDD_OK;
}

// Diagnostic: mdd_beam through the stamped instantiation of the single-wave kernel, its phase cycle sums into the caller's own
// stamps_dev [B,12].  A shape the plan sends to the generic kernel (MDD_BEAM_GENERIC included), or no buffer, is refused like any bad argument.
extern "C" int mdd_diag_beam_stamps(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, int32_t beam,
                                    int32_t blank, const double *lm_dev, double lm_alpha, int32_t *ids_dev, int32_t *nids_dev,
                                    int32_t *status_dev, double *score_dev, long long *stamps_dev, void *stream) {
    return beam_search({"mdd_diag_beam_stamps", false, true, logp_dev, T, B, C, len_dev, beam, blank, lm_dev, lm_alpha, 0, ids_dev, nids_dev, status_dev,
                        score_dev, stamps_dev, (hipStream_t)stream});
}
