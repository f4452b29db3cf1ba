// fp64 value, fp32 increment log-adds of the CTC lattices (ctc.hip's header comment; shared by ctc.hip, ctc_variants.hip and ctc_confnet.hip):
//   m + log(sum exp(x - m)),  the differences and the exp / log in fp32 on the hardware transcendental units (v_exp_f32 / v_log_f32, 1 ulp).
// The terms are <= 1 and the largest is exactly 1, so one log-add's absolute error is ~1e-7 whatever the magnitude of the values.
// All-(-inf) operands give -inf, never NaN.
#pragma once
#include <hip/hip_runtime.h>

namespace mdd {

__device__ __forceinline__ float fexp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
__device__ __forceinline__ float flog(float x) { return __builtin_amdgcn_logf(x) * 0.693147180559945309417f; }
__device__ __forceinline__ double wlse2(double a, double b) {
    const double m = fmax(a, b);
    const double mm = (m == -INFINITY) ? 0.0 : m;
    const float s = fexp((float)(a - mm)) + fexp((float)(b - mm));
    return mm + (double)flog(s);
}
__device__ __forceinline__ double wlse3(double a, double b, double c) {
    const double m = fmax(a, fmax(b, c));
    const double mm = (m == -INFINITY) ? 0.0 : m;
    const float s = fexp((float)(a - mm)) + fexp((float)(b - mm)) + fexp((float)(c - mm));
    return mm + (double)flog(s);
}

}  // namespace mdd
