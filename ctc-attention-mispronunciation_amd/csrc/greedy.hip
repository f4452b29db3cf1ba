// CTC decoders on the GPU: greedy (the prefix beam search: beam.hip).
//
// Reference: GreedyDecoder.decode (AA/utils/ctcDecoder.py:188-200 + :80-92).  Like the beam search it is a serial scan over the posterior
// frames of one utterance, latency-bound, not bandwidth- or flop-bound (180 B read per frame).  One workgroup per utterance.
#include "mdd_internal.h"

namespace mdd {

// argmax per frame (a wave per frame, first index wins ties like torch.max on CPU), then collapse:
// drop an element equal to its immediate predecessor (blank included in the comparison), drop blanks.
__global__ __launch_bounds__(256) void greedy_kernel(const float *__restrict__ logp, int T, int B, int C,
                                                     const int32_t *__restrict__ len, int blank,
                                                     int32_t *__restrict__ ids, int32_t *__restrict__ nids) {
    extern __shared__ int am[];  // [T]
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int n = len[b];
    n = n < 0 ? 0 : (n > T ? T : n);
    for (int t = wave; t < n; t += 4) {
        const float *row = logp + ((size_t)t * B + b) * C;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int c = lane; c < C; c += 64) {
            float v = row[c];
            if (v > bv || bi == 0x7fffffff) { bv = v; bi = c; }  // strict >: first index wins within a lane
        }
        for (int o = 32; o > 0; o >>= 1) {
            float ov = __shfl_xor(bv, o);
            int oi = __shfl_xor(bi, o);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
        }
        if (lane == 0) am[t] = bi;
    }
    __syncthreads();
    if (wave != 0) return;
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int t = base + lane;
        bool keep = false;
        int a = 0;
        if (t < n) {
            a = am[t];
            keep = (a != blank) && !(t != 0 && a == am[t - 1]);
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) ids[(size_t)b * T + count + __popcll(mask & ((1ull << lane) - 1ull))] = a;
        count += __popcll(mask);
    }
    if (lane == 0) nids[b] = count;
}

}  // namespace mdd

extern "C" int mdd_greedy(const float *logp_dev, int32_t T, int32_t B, int32_t C, const int32_t *len_dev, int32_t blank,
                          int32_t *ids_dev, int32_t *nids_dev, void *stream) {
    using namespace mdd;
    if (!logp_dev || !len_dev || !ids_dev || !nids_dev || T <= 0 || B <= 0 || C <= 0 || blank < 0 || blank >= C) {
        set_error("mdd_greedy: bad argument"); return MDD_ERR_ARG;
    }
    if ((size_t)T * 4 > 150 * 1024) { set_error("mdd_greedy: T=%d too long", T); return MDD_ERR_ARG; }
    hipLaunchKernelGGL(greedy_kernel, dim3(B), dim3(256), (size_t)T * sizeof(int), (hipStream_t)stream, logp_dev, T, B, C,
                       len_dev, blank, ids_dev, nids_dev);
    MDD_LAUNCH_CHECK();
    return MDD_OK;
}
