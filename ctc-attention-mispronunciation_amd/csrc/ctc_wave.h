// Wave-level device helpers of the CTC lattice kernels (ctc.hip, ctc_align.hip, ctc_confnet.hip, ctc_confnet_best.hip), beside ctc_lse.h.
#pragma once
#include <hip/hip_runtime.h>

namespace mdd {

// LDS traffic of ONE wave is processed in order; this only keeps the compiler from moving accesses across the point
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// lane i <- lane i-1 (SHR) / lane i+1 (SHL) across the whole wave; the edge lane gets -inf
static constexpr int DPP_WAVE_SHL1 = 0x130, DPP_WAVE_SHR1 = 0x138;
template <int CTRL>
__device__ __forceinline__ double wave_shift(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int lo2 = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    const int hi2 = __builtin_amdgcn_update_dpp((int)0xfff00000, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi2, lo2);
}
template <int CTRL>
__device__ __forceinline__ float wave_shift(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp((int)0xff800000, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// Two sums over the 64 lanes, every lane returning the same bits.  They add in DIFFERENT orders, so they round differently: they are two
// functions and neither may stand in for the other.
// wave_sum_dpp: within rows of 16 by DPP (quad_perm, row_half_mirror, row_mirror), then the four row sums in ascending order.  The bits of
// ctc_wave_kernel's gradient (the blank class) depend on this order, not wave_sum_butterfly's.
__device__ __forceinline__ float wave_sum_dpp(float x) {
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xf, 0xf, true));   // row_half_mirror
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xf, 0xf, true));   // row_mirror
    const int xi = __builtin_bit_cast(int, x);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 0)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 16)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 32)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 48));
}
// wave_max_dpp: the maximum of a double over the 64 lanes, every lane returning the same bits, by wave_sum_dpp's route (rows of 16 by DPP,
// then the four row maxima).  A maximum does not depend on the order, so it is the butterfly's value without its twelve ds_bpermutes.
template <int CTRL>
__device__ __forceinline__ double wave_dpp_all(double v) {      // CTRL must name a source for every lane (quad_perm, row mirrors)
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_max_dpp(double x) {
    x = fmax(x, wave_dpp_all<0xB1>(x));     // quad_perm [1,0,3,2]
    x = fmax(x, wave_dpp_all<0x4E>(x));     // quad_perm [2,3,0,1]
    x = fmax(x, wave_dpp_all<0x141>(x));    // row_half_mirror
    x = fmax(x, wave_dpp_all<0x140>(x));    // row_mirror
    const int lo = __double2loint(x), hi = __double2hiint(x);
    double r[4];
    for (int q = 0; q < 4; q++) r[q] = __hiloint2double(__builtin_amdgcn_readlane(hi, 16 * q), __builtin_amdgcn_readlane(lo, 16 * q));
    return fmax(fmax(r[0], r[1]), fmax(r[2], r[3]));
}
// wave_sum_butterfly: __shfl_xor over distances 32, 16, .., 1.  The bits of ctc_confnet_kernel's log-adds (lse_all, excl_all) depend on this
// order, not wave_sum_dpp's.
__device__ __forceinline__ float wave_sum_butterfly(float v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace mdd
